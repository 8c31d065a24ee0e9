// omc_ctx.h -- private to libomc.so (not installed, not part of include/omc.h): the context, its device buffers and
// the helpers the omc_api*.hip files share.  Definitions in omc_api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/omc.h"
#include "../../include/omc_jump_bounds.h"
#include "omc_basket.h"
#include "omc_bounds.h"
#include "omc_comm.h"
#include "omc_jump.h"
#include "omc_kernels.h"
#include "omc_p2p.h"

namespace omc::abi {

extern thread_local std::string g_err;  // omc_last_error()

inline int fail(int code, const char* msg)
{
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            char buf_[256];                                                                \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                     __FILE__, __LINE__);                                                  \
            g_err = buf_;                                                                  \
            return (int)e_ > 0 ? (int)e_ : 999;                                            \
        }                                                                                  \
    } while (0)

// Option "alloc_limit" (omc_set_option; per process, 0 = none): a single buffer of the library may not grow beyond this many
// bytes -- a request above it fails like a hipMalloc that found no room (hipErrorOutOfMemory).  A memory budget for a
// card shared with other tenants, and the way the tests make ONE rank of a job run out of memory.
extern size_t g_alloc_limit;

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return 0;
        if (g_alloc_limit && bytes > g_alloc_limit) {
            g_err = "hipMalloc refused: " + std::to_string(bytes) + " bytes asked for, option alloc_limit is " +
                    std::to_string(g_alloc_limit) + " (out of memory)";
            return (int)hipErrorOutOfMemory;
        }
        if (p) {
            hipError_t e = hipFree(p);
            p = nullptr;
            cap = 0;
            if (e != hipSuccess) return (int)e;
        }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {  // no room for the 12.5 % growth slack: ask for exactly what is needed
            (void)hipGetLastError();
            want = bytes;
            e = hipMalloc(&p, want);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();  // a failed hipMalloc must not surface at the next launch's hipGetLastError()
            g_err = std::string("hipMalloc failed: ") + hipGetErrorString(e);
            p = nullptr;
            return (int)e;
        }
        cap = want;
        return 0;
    }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;  // owns its allocation
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// argument checks: 0, or the error code with omc_last_error() set
int check_market(double S0, double K, double T, double r);
int check_sizes(int64_t n_paths, int n_steps);
int check_matrix(const void* S, int64_t ld, int64_t n_paths);
int check_lsm_args(const void* S, int64_t ld, int64_t n_paths, int n_steps, double K, double r, double T);
int check_params(const omc_params* p);
// the checks of a chain's own arguments (omc_api_chain.hip); `e` may be null when only p and n are to be judged
int check_chain(const omc_ctx* c, const omc_params* p, const omc_chain_entry* e, int n);
// a Heston scheme (0 .. 3, else -4) and what it needs of the law: OMC_HESTON_QE divides by kappa and xi and needs a positive
// long-run mean (-36)
int check_heston_scheme(int scheme, double kappa, double theta, double xi);
int check_contnet(omc_ctx* c, int hidden, int epochs, double lr);

// streams, workspace, collectives
int bind(omc_ctx* c);
int bind_in(omc_ctx* c);
int wait_stream(omc_ctx* c);
int prepare_lsm(omc_ctx* c, int64_t M, int N, double r, double T, bool two_pass, bool clear_tables, omc::LsmWorkspace* w);
int ensure_discounts(omc_ctx* c, int N, double r, double T, double** D);  // the context's table exp(-r dt k), k = 0 .. N
int allreduce(omc_ctx* c, double* dptr, int count);
int allreduce_host(omc_ctx* c, double* dev, double* host, int n);
bool p2p_active(const omc_ctx* c);
bool step_graph_enabled(const omc_ctx* c);
int adam_bias_tables(omc_ctx* c, double beta1, double beta2, size_t need, size_t cap);
int enqueue_lsm(omc_ctx* c, const omc::LsmProblem& p, const omc::LsmWorkspace& w, int semantics, bool write_state);
int check_p2p(omc_ctx* c, const double* h = nullptr, int n = 0);

// results, device scratch layouts
void fill_result(omc_result* res, const double* h, int64_t M, int world = 1);  // clears *res first
int copy_outputs(omc_ctx* c, const omc::LsmWorkspace& w, int64_t M, int N, double* betas_out, float* sx_out,
                 int32_t* tex_out);
// the caller's fits [N+1][4] into w.betas; returns once they are copied (`betas` is caller memory)
int upload_fits(omc_ctx* c, const omc::LsmWorkspace& w, const double* betas, int N);
// the mean of M samples from their sum and sum of squares, and its standard error
inline void mean_and_se(double s, double s2, double M, double* mean, double* se)
{
    *mean = s / M;
    const double var = s2 / M - *mean * *mean;
    *se = std::sqrt((var > 0.0 ? var : 0.0) / M);
}
inline size_t up256(size_t bytes) { return (bytes + 255) / 256 * 256; }  // the next block of a scratch layout

// the library's own path matrix and the fused pricing
inline int64_t padded_ld(int64_t cols) { return (cols + 63) / 64 * 64; }  // leading dimension of a matrix it owns
enum class Storage { planned, full_only };  // plan_storage's choice, or the full matrix whatever the pricing
int enqueue_paths(omc_ctx* c, const omc_params* p, float* S, int64_t ld, bool fold = false);
bool fold_applies(const omc_ctx* c, const omc_params* p);
int plan_storage(omc_ctx* c, const omc_params* p, int slot, int64_t* ld, const double** cK);
int ensure_paths(omc_ctx* c, const omc_params* p, Storage how, float** S, int64_t* ld, const double** cK = nullptr);
// gen: the parameters the generator and the fold table take (null: p; a dividend yield hands p with r - q as its rate)
int enqueue_pricing(omc_ctx* c, const omc_params* p, float* S_keep, int64_t ld, double* result_dev, hipEvent_t* evs,
                    double** result_out, const omc_params* gen = nullptr);
int price_fused(omc_ctx* c, const omc_params* p, const omc_params* gen, omc_result* res, float* S_keep, int64_t ld);
int read_kernel_times(const hipEvent_t* evs, const omc_params* p, omc_result* res, bool has_end = true);

// ---- a generator of its own that writes a full-storage matrix, then the unchanged two-pass sweeps (dividends, jumps,
// multi-asset, barrier): DESIGN.md section 14, "adding a generator"
// which paths: `p` with `drift_rate` as the rate of the paths, the width hint of p's model, the matrix S [N+1][ld]
omc::PathSpec path_spec(const omc_ctx* c, const omc_params* p, double drift_rate, float* S, int64_t ld);
// the same law at other paths: n_paths of them at (p->seed, stream, pair_offset)
omc::PathSpec path_spec(const omc_ctx* c, const omc_params* p, double drift_rate, float* S, int64_t ld, int64_t n_paths,
                        uint64_t stream, uint64_t pair_offset);
// the matrix the generator writes: the caller's S_keep (refusal -6 when *ld < n_paths) or the context's own, in full
int take_full_matrix(omc_ctx* c, const omc_params* p, float* S_keep, float** S, int64_t* ld);
// events 0 and 1 around gen(stream), the two-pass flow on S with its pass events, event 2, the eight sums -> c->hres
int enqueue_generated(omc_ctx* c, const omc_params* p, const float* S, int64_t ld,
                      const std::function<hipError_t(hipStream_t)>& gen);
// waits for the stream; *base from c->hres (full storage: folded = 0) with the kernel times
int finish_generated(omc_ctx* c, const omc_params* p, omc_result* base);

// ---- multi-asset options: what omc_price_american_basket and omc_price_american_basket_bounds share (omc_api_basket.hip)
struct BasketTable {
    int d;
    double L[omc::kBasketTri];  // packed lower triangle: row i at i (i + 1) / 2
    float a[omc::kBasketMax], b[omc::kBasketMax];
    double x0, G0, sigma_G, q_G;
};
// the argument checks of include/omc.h's multi-asset section and the host constants: 0, or the code with the message set
int compose_basket(const omc_params* p, const omc_basket* k, BasketTable* t);
omc::BasketLaw basket_law(const BasketTable& t, const omc_basket* k);  // what the kernels take by value

// ---- jump-diffusion: what omc_price_american_jump, omc_jump_paths_f32 and omc_price_american_bounds_jump share
// (omc_api_jump.hip)
struct JumpTable {
    uint32_t thr[omc::kJumpThr];
    double kappa, drift_rate;
    int n_thr;  // entries below 2^24
};
// the argument checks of include/omc.h's jump-diffusion section and the host side of the law: 0, or the code with the
// message set.  priced: the two-pass pricing's semantics check (-11); start_state: p->v0 of Heston schemes 0 .. 2 is a
// stored state and is not validated
int compose_jump(const omc_params* p, const omc_jump* j, double q, JumpTable* t, bool priced, bool start_state);
omc::JumpLaw jump_law(const JumpTable& t, const omc_jump* j);  // what the kernels take by value

// ---- Andersen-Broadie bounds: the flow omc_price_american_bounds and omc_price_american_basket_bounds share
// (omc_api_bounds.hip).  The caller has checked its params; what differs between one asset and several is where the
// paths come from and which kernels simulate the fresh ones.
struct BoundsFlow {
    int d = 1;               // assets: an inner launch covers at most 2^30 / d worst-case inner path steps
    size_t extra_bytes = 0;  // room in the workspace beside the outer matrix (the outer asset matrices)
    // the paths of p (the policy fit's) into S [N+1][ld], on the context's stream
    std::function<int(float* S, int64_t ld)> fit_paths;
    // called once, before anything is enqueued: the common arguments are filled, `extra` is the caller's room
    std::function<void(const omc::BoundsArgs& a, char* extra)> bind;
    std::function<hipError_t(hipStream_t, double* result)> lower;
    std::function<hipError_t(hipStream_t)> outer;  // the outer paths into a.So (and what the caller keeps in `extra`)
    std::function<hipError_t(hipStream_t, int64_t i0, int64_t ni)> inner;
    // The schedule (option "bounds_exercise_every" = k >= 2; default: none).  A flow that sets it takes
    // the context's schedule -- Q^ at the scheduled dates only, with run_bounds' own fit on the gathered rows and walk over
    // the scheduled dates -- and one that leaves it empty is refused (-38) while the option holds a schedule.
    std::function<hipError_t(hipStream_t, const omc::BoundsSched& sc, int64_t i0, int64_t ni)> inner_sched;
    // The control variate (option "bounds_control_variate" = 1; default: none).  A flow that sets
    // lower_cv, inner_cv and (to take a schedule too) inner_sched_cv is run with them in the place of lower, inner and
    // inner_sched while the option is on: lower_cv leaves the sums of the CENTRED pair means, to whose mean run_bounds adds
    // cv_e0, and inner_cv writes the controlled Q^.  One that leaves them empty is refused (-39) while the option is on.
    std::function<hipError_t(hipStream_t, double* result)> lower_cv;
    std::function<hipError_t(hipStream_t, int64_t i0, int64_t ni)> inner_cv;
    std::function<hipError_t(hipStream_t, const omc::BoundsSched& sc, int64_t i0, int64_t ni)> inner_sched_cv;
    double cv_e0 = 0.0;  // E0 = D[0] E(S0, 0), float64 on the host
    // Sub-optimality checking (option "bounds_suboptimality" = m >= 1; default: off).  A flow that sets
    // inner_check is run with it in the place of inner -- Q^ at the items of run_bounds' kept list only -- and, with the
    // control variate on, with inner_check_cv in the place of inner_cv.  euro_table (mode 2) leaves the table of E's
    // per-date constants on the device, built if the call has not built it yet, and returns it.  A flow that leaves what the
    // option asks for empty is refused (-40), as is every flow with a policy of its own.
    std::function<hipError_t(hipStream_t, const omc::BoundsCheck& k, int64_t i0, int64_t ni)> inner_check;
    std::function<hipError_t(hipStream_t, const omc::BoundsCheck& k, int64_t i0, int64_t ni)> inner_check_cv;
    std::function<hipError_t(hipStream_t, const double** cv)> euro_table;
    // Items the law itself takes out (a knock-out's dead items; default: none).  A flow that sets
    // mark_items and inner_check runs the all-dates game list-driven even while the sub-optimality option is off: mark_items
    // writes bounds_check_mark's outputs (k.mode is 0) by its own rule, the list, inner_check and the walk over the kept
    // dates are section 27's.  With the option on the mark is bounds_check_mark's, with a schedule the flow is not used.
    std::function<hipError_t(hipStream_t, const omc::BoundsCheck& k)> mark_items;
    // A policy of the flow's own (omc_api_runnerup_bounds.hip: a rule on two regressors), all three set or none.  With them
    // run_bounds neither uploads nor fits a [N+1][4] table and builds no exercise tables:
    //   own_policy(w, S, ld)   between the fit events: the caller's table to the device (S == nullptr), or the fit on the
    //                          p->n_paths paths it writes itself into S [N+1][ld]; w.sx, w.tex, w.D are its to use
    //   walk                   in the place of bounds_walk
    //   read_policy            the policy used into the caller's betas_out (enqueued; run_bounds waits for the stream)
    std::function<int(const omc::LsmWorkspace& w, float* S, int64_t ld)> own_policy;
    std::function<hipError_t(hipStream_t, double* result)> walk;
    std::function<hipError_t(hipStream_t, double* betas_out)> read_policy;
};
// the cfg checks (-10, -4, -7, -3, -16), the policy, the sweeps, the walk, the read-back and *out
int run_bounds(omc_ctx* c, const omc_params* p, const omc_bounds_config* cfg, const double* betas, double* betas_out,
               double* q_out, double* samples_out, omc_bounds* out, const BoundsFlow& f);
// The hooks of a one-asset law whose policy sees the spot (Heston, jump-diffusion, dividends): the normals per step, the room
// for the outer variance state under Heston, the binding of `a` and of the diffusion's Vo, and the four sweeps through the
// overloads of bounds_lower / bounds_inner / bounds_check_inner / bounds_sched_inner for `law`, whose diffusion `d` is (or is
// law itself).  a, law and d outlive the flow's run; fit_paths and outer stay the caller's.  (The calls are unqualified: the
// law's overloads are declared in its own header and found through the arguments' namespace.)
template <class Law>
void one_asset_flow(BoundsFlow& f, omc::BoundsArgs& a, Law& law, omc::DiffusionLaw& d, const omc_params* p,
                    const omc_bounds_config* cfg)
{
    const bool heston = d.model != 0;
    f.d = heston ? 2 : 1;  // normals per step
    if (heston && cfg->n_outer > 0)  // (sizes are checked in run_bounds, before the room is used)
        f.extra_bytes = sizeof(float) * (size_t)(p->n_steps + 1) * (size_t)cfg->n_outer;
    f.bind = [&a, &d, p, heston](const omc::BoundsArgs& common, char* extra) {
        a = common;
        a.s0 = (float)p->S0;  // the generator's start value, so every spot is the generator's
        d.Vo = heston ? (const float*)extra : nullptr;
    };
    f.lower = [&a, &law](hipStream_t st, double* res) { return bounds_lower(st, a, law, res); };
    f.inner = [&a, &law](hipStream_t st, int64_t i0, int64_t ni) { return bounds_inner(st, a, law, i0, ni); };
    f.inner_check = [&a, &law](hipStream_t st, const omc::BoundsCheck& k, int64_t i0, int64_t ni) {  // section 27: the payoff check
        return bounds_check_inner(st, a, law, k, i0, ni);
    };
    f.inner_sched = [&a, &law](hipStream_t st, const omc::BoundsSched& sc, int64_t i0, int64_t ni) {
        return bounds_sched_inner(st, a, law, sc, i0, ni);
    };
}

// ---- K two-pass pricings of one geometry that share their small launches (grouped sequences, option chains)
// device bytes one member of a group owns in omc_ctx::gstate: [part1 | gmom | betas | crit | part]
struct GroupLayout {
    size_t o_gmom, o_betas, o_crit, o_part, per;
    GroupLayout(int64_t M, int N);
};
// One group on a stream.  The caller adds its members, enqueues their sweeps from prob[k] / w[k] (lsm_pass1_sweep into
// &g.ntiles, lsm_pass2_sweep into &g.nblk, or the chain's fused ones) and places the three shared launches between them:
//     pass-1 sweeps;  reduce_pass1;  build_tables (members that decide from tables);  pass-2 sweeps;  finalize
struct TwoPassGroup {
    // `state`: room for L.per bytes per member; w0: the members' template (discount table, gstride, crit_irr_every,
    // part1_tiles); tables: pass 2 decides from exercise tables (option "pass2_tables"), else the members carry none
    TwoPassGroup(const GroupLayout& L, void* state, const omc::LsmWorkspace& w0, bool tables);
    void add(const omc::LsmProblem& p, double* result);  // the next member, k = K
    hipError_t reduce_pass1(hipStream_t st) const { return omc::lsm_group_reduce_pass1(st, g, K); }
    hipError_t build_tables(hipStream_t st) const { return omc::lsm_group_crit_build(st, g, K); }  // folded members only
    hipError_t finalize(hipStream_t st) const { return omc::lsm_group_finalize(st, g, K); }
    int K = 0;
    omc::LsmProblem prob[omc::kSeqGroupMax];
    omc::LsmWorkspace w[omc::kSeqGroupMax];
    omc::SeqGroupArgs g = {};

private:
    GroupLayout L;
    char* state;
    omc::LsmWorkspace w0;
    bool tables;
};

}  // namespace omc::abi

using omc::abi::DevBuf;

// What the count call of omc_nn_build_rows (data == NULL) leaves for the call with `data` that follows it: the sweep's
// results on the host, the counts / offsets in the context's scratch.  Valid only for the NEXT library call on the context
// (every entry point clears it in bind()), and only for the same arguments.
struct RowsCache {
    bool valid = false;
    const float* S = nullptr;
    int64_t ld = 0, M = 0;
    int N = 0, is_put = 0;
    double K = 0, r = 0, T = 0;
    int64_t R = 0;
    double st[16] = {0};
};

constexpr size_t kVoteBytes = 1024;  // omc_ctx::seq_vote once a communicator / hook is installed (largest use: 40 doubles)

struct omc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DevBuf S, sx, tex, ex, D, part, gmom, betas, part1, result, scratch, sweep_args, crit;
    DevBuf bslab, btable, bres, bdisc;  // batched path: problem slab, table, results, discounts
    DevBuf mlp_part, mlp_loss, mlp_wt;  // NN training: gradient partials, epoch loss, transposed connections
    DevBuf mlp_gred, shard;             // sharded NN training: reduced gradient of a step; epoch selection tables
    DevBuf cn_scratch, cn_data, cn_net, cn_cont;  // per-step ContNet flow: set bookkeeping, rows, net + Adam state, values
    std::vector<char> h_table;
    std::vector<double> h_disc, h_bres;
    std::vector<double> hD;
    int D_N = -1;
    double D_r = 0, D_T = 0;
    const double* D_ptr = nullptr;
    double hres[8];
    double* hres_pin = nullptr;  // pinned + mapped: the fused pricing call's last kernel writes its 8 sums here
    double* hres_dev = nullptr;  // device-side address of hres_pin
    double *seq_pin = nullptr, *seq_dev = nullptr;  // omc_price_american_seq: one 8-double slot per pricing
    int seq_cap = 0;
    hipEvent_t ev_seq = nullptr;
    hipEvent_t ev_entry = nullptr;  // bind_in(): orders a context-owned stream after the device's default stream
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // omc_price_american_seq: further event sets (7 each) for the pricings of a sequence that carry their own
    // kernel timings ("seq_event_stride": every k-th pricing; 0 = the first one only)
    std::vector<hipEvent_t> ev_pool;
    int seq_event_stride = 0;
    // omc_price_american_seq, per-step flows: K pricings advanced by one launch per time step
    DevBuf mS, mstate, mtable;
    DevBuf mb_slab, mb_table, mb_bc;      // omc_mlp_train_epoch_batch: per-problem scratch, table, 1 - beta^step tables
    std::vector<double> mb_bc_host;       // [2][cap]: bc1 then bc2
    double mb_beta1 = -1.0, mb_beta2 = -1.0;
    size_t mb_bc_cap = 0;
    char* mtab_pin = nullptr;  // pinned upload ring for the argument tables (one image per batch of K)
    int mtab_slot = 0;
    int seq_step_k = -1;       // -1: default (what fits the Infinity Cache, <= 16), 1: off, k: at most k pricings per launch
    int seq_step_wgs = 0;      // workgroups one launch of the multi-pricing sweep may use (0: one per CU)
    // groups of K two-pass pricings of one geometry whose pass-1 reductions, table builds and finalizes share three
    // launches (TwoPassGroup): gstate = per member of a group [part1 | gmom | betas | crit | part] (GroupLayout), for
    // omc_price_american_seq's groups and omc_price_american_chain's alike; gS = the sequence's K path matrices
    DevBuf gS, gstate;
    int seq_two_pass_k = -1;   // -1: by size (omc_api_seq.hip), 1: one pricing at a time, k: at most k pricings per group
    int gbm_vec = 0, heston_vec = 0;
    // antithetic-folded storage of the fused GBM two-pass pricing (omc_lsm_dev.h; option "fold_antithetic": 0 never,
    // 1 = default: pricings of at least kFoldMinPaths paths over all ranks, 2 always): two cK tables (the overlapped
    // sequence has two pricings in flight), each remembered by what it was filled from
    int fold = 1;
    // pass 2 of the two-pass flow decides from per-step float32 exercise tables (option "pass2_tables": 1 = default,
    // 0 = the float64 decisions; the same decisions either way)
    int pass2_tables = 1;
    int pass2_irr_every = 0;  // tests (option "pass2_tables_irregular_every"): every k-th step decided by the float64 fallback
    DevBuf foldC;
    DevBuf gk_part, gk_res;  // omc_price_american_greeks: per-workgroup partials, reduced sums
    DevBuf bar_part, bar_res;  // omc_price_barrier: the generator's per-workgroup partials, reduced sums
    DevBuf div_tab;            // omc_price_american_div: the dividend steps of the call (omc::DivEntry)
    int64_t bounds_every = 0;  // option "bounds_exercise_every": 0 / 1 every date, k >= 2 the bounds of the scheduled game
    int bounds_cv = 0;         // option "bounds_control_variate": 1 = the GBM bounds' Black-Scholes control variate (section 26)
    int bounds_cv_form = 0;    // option "bounds_cv_form" (tests, measurement): omc::kCvFormDefault / kCvFormWave
    int bounds_subopt = 0;     // option "bounds_suboptimality": 0 off, 1 payoff, 2 European (sub-optimality checking, section 27)
    DevBuf bnd;                // omc_price_american_bounds: outer paths, Q^ table, samples, tables, partials, sums
    DevBuf chain_fold;         // omc_price_american_chain: the entries' fold tables + c0 (their small buffers: gstate)
    DevBuf chain_sched;        // ... and its Bermudan entries' tables on their scheduled dates (omc::chain_schedule_tables)
    int chain_fused = 0;       // option "chain_fused": 0 = default, the single-strike sweeps per entry; 1 = the fused sweeps
    int chain_k = -1;          // option "chain_k": entries per fused launch at most (-1: what omc_chain.hip allows)
    // omc_price_american_chain_greeks: the entries' slots, per-workgroup partials of a group, reduced sums of every entry;
    // the host images of the slots and of the caller's policies (pageable: kept until the call's wait)
    DevBuf cg_slots, cg_part, cg_res;
    std::vector<char> cg_hslots;
    std::vector<double> cg_hgiven, cg_hview, cg_hres;  // ... and of the fits and the sums it reads back
    int chain_greeks_k = -1;      // option "chain_greeks_k": entries per Greeks sweep launch (-1: 16)
    int chain_greeks_order = 0;   // option "chain_greeks_order" (measurement): omc::kChainGreeksBanded / kChainGreeksPlain
    struct FoldKey { int N = -1; double c0 = 0, g = 0; } fold_key[2];
    int world = 1;  // ranks whose sums the hook / communicator adds up (equal shards)
    omc_allreduce_fn hook = nullptr;
    void* hook_user = nullptr;
    omc::Comm* comm = nullptr;  // native RCCL communicator (omc_comm_init); takes precedence over the hook
    // direct write-to-all-peers exchange of the per-step moments (omc_p2p_connect): replaces the per-step all-reduce
    omc::P2P* p2p = nullptr;
    int p2p_use = 1;            // option "p2p_exchange": 0 = keep the collective even when connected
    bool p2p_used = false;      // an exchange was enqueued since the last wait
    double p2p_deadline_s = 2.0;  // option "p2p_deadline_ms": how long an exchange waits for a peer's contribution
    double p2p_first_deadline_s = 30.0;  // "p2p_first_deadline_ms": the same for the FIRST exchange of a call
    // omc_price_american_seq across GPUs: the moment all-reduce of pricing k runs on its own stream while the
    // main stream generates the paths of pricing k+1 into the second path buffer
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_moments[2] = {nullptr, nullptr}, ev_reduced[2] = {nullptr, nullptr};
    RowsCache rows_cache;
    DevBuf S2, seq_local, part1b, gmomb, seq_vote;
    int seq_overlap = -1;  // -1: default (on when the communicator has more than one rank), 0 off, 1 on
    bool defer_result_allreduce = false;  // inside omc_price_american_seq: one collective for all result sums
    // captured per-step sweep (N launches + valuation + finalize), replayed for every pricing of the
    // same geometry; its kernels read their arguments from `sweep_args`
    hipGraph_t sweep_graph = nullptr;
    hipGraphExec_t sweep_exec = nullptr;
    int64_t sg_M = -1, sg_ld = -1;
    int sg_N = -1, sg_sem = -1, sg_vec4 = -1, sg_failed = 0;
    const void* sg_args = nullptr;
    std::vector<char> sweep_img;   // last argument image uploaded to sweep_args
    char* sweep_pin = nullptr;     // pinned upload ring
    int sweep_pin_slot = 0;
    int step_graph = -1;           // -1: environment default (off), 0 off, 1 on
    int device_cus = 0;
    bool distributed() const { return comm != nullptr || hook != nullptr; }
    ~omc_ctx();  // releases everything it holds (omc_api.hip)
};

