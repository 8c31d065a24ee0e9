// omc_api.hip -- the C ABI of libomc.so (include/omc.h): the helpers the entry points share (argument checks,
// launch sequencing, HIP-event timing), contexts, memory, options, the all-reduce hook, RCCL and the direct peer
// exchange.  The other entry points live in omc_api_{price,seq,batch,nn,bounds,chain,dividend}.hip; omc_ctx.h is their common ground.
// No kernel code here.
#include <sched.h>

#include <algorithm>

#include "omc_ctx.h"

namespace omc::abi {

thread_local std::string g_err;
size_t g_alloc_limit = 0;

int check_market(double S0, double K, double T, double r)
{
    if (!(S0 > 0) || !(K > 0) || !(T > 0)) return fail(-1, "S0, K, T must be positive.");
    if (!(r >= 0)) return fail(-2, "r must be non-negative.");
    return 0;
}

int check_sizes(int64_t n_paths, int n_steps)
{
    if (n_paths <= 0 || n_steps <= 0)
        return fail(-3, "num_simulations and num_time_steps must be positive integers.");
    if (n_steps > omc::kMaxSteps) return fail(-8, "num_time_steps exceeds the supported maximum (4094).");
    return 0;
}

int check_matrix(const void* S, int64_t ld, int64_t n_paths)
{
    if (!S) return fail(-7, "null path matrix pointer.");
    if (ld < n_paths) return fail(-6, "leading dimension smaller than n_paths.");
    return 0;
}

// a backward induction on the caller's path matrix
int check_lsm_args(const void* S, int64_t ld, int64_t n_paths, int n_steps, double K, double r, double T)
{
    int rc;
    if ((rc = check_market(1.0, K, T, r))) return rc;
    if ((rc = check_sizes(n_paths, n_steps))) return rc;
    return check_matrix(S, ld, n_paths);
}

int bind(omc_ctx* c)
{
    if (!c) return fail(-7, "null context.");
    c->rows_cache.valid = false;  // (omc_nn_build_rows looks at it before it gets here)
    HIP_TRY(hipSetDevice(c->device));
    return 0;
}

// Entry of every call that takes BORROWED device pointers.  A context that owns its stream creates it with
// hipStreamNonBlocking, so nothing orders it after work the caller still has in flight on the device's default
// (null) stream -- which is where PyTorch queues the torch.full / torch.empty / copy that produced the pointer.
// Record a marker on the null stream and make the context's stream wait for it: asynchronous, a few microseconds
// of host time, and the caller's producer is then always ahead of the library's consumer.  A context that borrows
// the caller's stream is ordered by that stream itself.  (Work on OTHER caller streams is the caller's to order:
// include/omc.h, "stream ordering".)
int bind_in(omc_ctx* c)
{
    int rc = bind(c);
    if (rc) return rc;
    if (!c->own_stream) return 0;
    if (!c->ev_entry) HIP_TRY(hipEventCreateWithFlags(&c->ev_entry, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->ev_entry, nullptr));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_entry, 0));
    return 0;
}

// Wait for the stream by polling: a pricing lasts well under a millisecond, and the wake-up
// latency of a blocking hipStreamSynchronize is a visible fraction of that.  The spin is bounded
// in TIME (about 2 ms of polling, yielding the core between polls after the first 50 us), then the
// call blocks: several ranks on a small CPU quota must not burn it all in spin loops.
int wait_stream(omc_ctx* c)
{
    timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (int i = 0;; ++i) {
        const hipError_t q = hipStreamQuery(c->stream);
        if (q == hipSuccess) return 0;
        if (q != hipErrorNotReady) HIP_TRY(q);
        if ((i & 15) == 15) {
            clock_gettime(CLOCK_MONOTONIC, &t1);
            const double us = (t1.tv_sec - t0.tv_sec) * 1e6 + (t1.tv_nsec - t0.tv_nsec) * 1e-3;
            if (us > 2000.0) break;
            if (us > 50.0) sched_yield();
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// The context's discount table D[k] = exp(-r dt k), k = 0 .. N, for (N, r, T).
int ensure_discounts(omc_ctx* c, int N, double r, double T, double** D)
{
    int rc;
    if ((rc = c->D.ensure(sizeof(double) * (size_t)(N + 1)))) return rc;
    *D = (double*)c->D.p;
    // discount table computed on the host in double (same libm exp as the oracle); it only
    // depends on (N, r, T), so consecutive pricings of one contract reuse the device copy
    if (c->D_N != N || c->D_r != r || c->D_T != T || c->D_ptr != *D) {
        c->hD.resize((size_t)N + 1);
        const double dt = T / N;
        for (int k = 0; k <= N; ++k) c->hD[(size_t)k] = std::exp(-r * dt * (double)k);
        HIP_TRY(hipMemcpyAsync(*D, c->hD.data(), sizeof(double) * (size_t)(N + 1),
                               hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // hD is pageable host memory
        c->D_N = N; c->D_r = r; c->D_T = T; c->D_ptr = *D;
    }
    return 0;
}

// workspace for the backward induction on M paths x N steps
int prepare_lsm(omc_ctx* c, int64_t M, int N, double r, double T, bool two_pass,
                bool clear_tables, omc::LsmWorkspace* w)
{
    int rc;
    if ((rc = c->sx.ensure(sizeof(float) * (size_t)M))) return rc;
    if ((rc = c->tex.ensure(sizeof(int32_t) * (size_t)M))) return rc;
    if ((rc = c->ex.ensure(sizeof(float) * (size_t)M + 16))) return rc;
    if ((rc = c->part.ensure(sizeof(double) * 2 * 8 * omc::kMaxLsmBlocks))) return rc;
    if ((rc = c->gmom.ensure(sizeof(double) * 8 * (size_t)(N + 1)))) return rc;
    if ((rc = c->betas.ensure(sizeof(double) * 4 * (size_t)(N + 1)))) return rc;
    if ((rc = c->result.ensure(sizeof(double) * 8))) return rc;
    w->part1 = nullptr;
    w->part1_tiles = 0;
    w->crit = nullptr;
    if (two_pass && c->pass2_tables) {
        if ((rc = c->crit.ensure(sizeof(uint32_t) * 8 * (size_t)(N + 1)))) return rc;
        w->crit = (uint32_t*)c->crit.p;
    }
    w->crit_irr_every = c->pass2_irr_every;
    if (two_pass) {
        const size_t tiles = omc::lsm_part1_tiles(M);
        if ((rc = c->part1.ensure(sizeof(double) * 8 * (size_t)(N + 1) * tiles))) return rc;
        w->part1 = (double*)c->part1.p;
        w->part1_tiles = (int64_t)tiles;
    }
    w->sx = (float*)c->sx.p;
    w->tex = (int32_t*)c->tex.p;
    w->live = (float*)c->ex.p;
    w->part = (double*)c->part.p;
    w->gmom = (double*)c->gmom.p;
    w->betas = (double*)c->betas.p;
    w->result = (double*)c->result.p;
    if ((rc = ensure_discounts(c, N, r, T, &w->D))) return rc;
    // gmom rows 1..N-1, betas rows 1..N-1 and result[0..7] are fully written by the kernels of
    // every flow before anything reads them; rows 0 and N are only ever copied out, so they
    // are cleared just when the caller asked for the tables.
    if (clear_tables) {
        HIP_TRY(hipMemsetAsync(w->gmom, 0, sizeof(double) * 8 * (size_t)(N + 1), c->stream));
        HIP_TRY(hipMemsetAsync(w->betas, 0, sizeof(double) * 4 * (size_t)(N + 1), c->stream));
    }
    return 0;
}

// in-place sum over the ranks of `count` device doubles, ordered on the context's stream: the native
// RCCL communicator when there is one (enqueued from here, no host callback), else the caller's hook
int allreduce(omc_ctx* c, double* dptr, int count)
{
    if (c->comm) {
        std::string err;
        const int rc = omc::comm_allreduce_f64(c->comm, dptr, (size_t)count, 0, c->stream, &err);
        if (rc) return fail(rc, err.c_str());
        return 0;
    }
    if (c->hook) {
        if (c->hook(c->hook_user, dptr, count)) return fail(998, "all-reduce hook failed");
    }
    return 0;
}

// the same for `n` host doubles (n <= 8 * rows of `dev`, a device scratch of the caller's): up, all-reduce, down, wait
int allreduce_host(omc_ctx* c, double* dev, double* host, int n)
{
    int rc;
    HIP_TRY(hipMemcpyAsync(dev, host, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    if ((rc = allreduce(c, dev, n))) return rc;
    HIP_TRY(hipMemcpyAsync(host, dev, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// the per-step moments travel by direct peer writes instead of a collective: connected, switched on, and the same
// world as the communicator / hook the rest of the exchange uses
bool p2p_active(const omc_ctx* c)
{
    return c->p2p && c->p2p_use && omc::p2p_connected(c->p2p) && c->distributed() && omc::p2p_world(c->p2p) == c->world;
}

bool step_graph_enabled(const omc_ctx* c)
{
    if (c->step_graph >= 0) return c->step_graph != 0;
    // Off unless asked for: at 1M paths x 252 steps the replayed graph and the 254 plain launches take the
    // same time (1.563 vs 1.562 ms: the host was never the limiter), while every new geometry costs a
    // capture + instantiate of several milliseconds -- a curve whose points differ in step count would
    // pay that per point.
    static const int env = [] {
        const char* e = getenv("OMC_STEP_GRAPH");
        return e ? atoi(e) : 0;
    }();
    return env != 0;
}

static void drop_sweep_graph(omc_ctx* c)
{
    if (c->sweep_exec) (void)hipGraphExecDestroy(c->sweep_exec);
    if (c->sweep_graph) (void)hipGraphDestroy(c->sweep_graph);
    c->sweep_exec = nullptr;
    c->sweep_graph = nullptr;
    c->sg_M = -1;
}

// The per-step sweep as ONE graph launch.  Returns 0 when the sweep was enqueued, kNoGraph when the
// caller should launch the kernels one by one (capture unavailable), else an error code.
constexpr int kNoGraph = -12345;
static int enqueue_sweep_graph(omc_ctx* c, const omc::LsmProblem& p, const omc::LsmWorkspace& w, int semantics,
                               bool fill_state)
{
    if (c->sg_failed) return kNoGraph;
    const size_t nb = omc::lsm_sweep_args_bytes();
    constexpr int kSlots = 32;
    if (c->sweep_args.ensure(nb)) return kNoGraph;
    if (!c->sweep_pin && hipHostMalloc((void**)&c->sweep_pin, nb * kSlots, hipHostMallocDefault) != hipSuccess) {
        c->sweep_pin = nullptr;
        c->sg_failed = 1;
        (void)hipGetLastError();
        return kNoGraph;
    }
    std::vector<char> img(nb);
    omc::lsm_sweep_args_image(p, w, semantics, fill_state, img.data());
    if (img != c->sweep_img) {
        if (c->sweep_pin_slot == kSlots) {  // the ring wraps: earlier uploads must have been consumed
            HIP_TRY(hipStreamSynchronize(c->stream));
            c->sweep_pin_slot = 0;
        }
        char* slot = c->sweep_pin + nb * (size_t)c->sweep_pin_slot++;
        memcpy(slot, img.data(), nb);
        HIP_TRY(hipMemcpyAsync(c->sweep_args.p, slot, nb, hipMemcpyHostToDevice, c->stream));
        c->sweep_img.swap(img);
    }
    const int vec4 = omc::rows_aligned(4, p.M, p.S, p.ld) ? 1 : 0;  // the launcher's own rule (lsm_step_impl)
    if (!c->sweep_exec || c->sg_M != p.M || c->sg_N != p.N || c->sg_sem != semantics || c->sg_vec4 != vec4 ||
        c->sg_ld != p.ld || c->sg_args != c->sweep_args.p) {
        drop_sweep_graph(c);
        bool ok = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            const hipError_t le = omc::lsm_sweep_indirect(c->stream, p, w, semantics, c->sweep_args.p);
            const hipError_t ee = hipStreamEndCapture(c->stream, &c->sweep_graph);
            ok = le == hipSuccess && ee == hipSuccess && c->sweep_graph != nullptr;
        }
        if (ok) ok = hipGraphInstantiate(&c->sweep_exec, c->sweep_graph, nullptr, nullptr, 0) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            drop_sweep_graph(c);
            c->sg_failed = 1;
            return kNoGraph;
        }
        c->sg_M = p.M; c->sg_N = p.N; c->sg_sem = semantics; c->sg_vec4 = vec4; c->sg_ld = p.ld;
        c->sg_args = c->sweep_args.p;
    }
    HIP_TRY(hipGraphLaunch(c->sweep_exec, c->stream));
    return 0;
}

// Adam's bias corrections 1 - beta^k, k < cap, in c->mb_bc (bc1 then bc2; host libm pow: the numbers the single-network
// trainer uses), refilled when the betas change or fewer than `need` steps are covered
int adam_bias_tables(omc_ctx* c, double beta1, double beta2, size_t need, size_t cap)
{
    if (c->mb_beta1 == beta1 && c->mb_beta2 == beta2 && c->mb_bc_cap >= need) return 0;
    c->mb_bc_host.assign(2 * cap, 0.0);
    for (size_t k = 0; k < cap; ++k) {
        c->mb_bc_host[k] = 1.0 - std::pow(beta1, (double)k);
        c->mb_bc_host[cap + k] = 1.0 - std::pow(beta2, (double)k);
    }
    int rc;
    if ((rc = c->mb_bc.ensure(sizeof(double) * 2 * cap))) return rc;
    HIP_TRY(hipMemcpyAsync(c->mb_bc.p, c->mb_bc_host.data(), sizeof(double) * 2 * cap, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mb_bc_cap = cap; c->mb_beta1 = beta1; c->mb_beta2 = beta2;
    return 0;
}

// enqueue the whole backward induction on c->stream; sums land in w.result
int enqueue_lsm(omc_ctx* c, const omc::LsmProblem& p, const omc::LsmWorkspace& w, int semantics,
                bool write_state)
{
    hipStream_t st = c->stream;
    int rc;
    if (semantics == OMC_SEM_TWO_PASS) {
        HIP_TRY(omc::lsm_pass1_moments(st, p, w));
        if (c->distributed() && (rc = allreduce(c, w.gmom, 8 * (p.N + 1)))) return rc;
        HIP_TRY(omc::lsm_pass2_apply(st, p, w, write_state, true));  // solves the fits itself
    } else {
        const bool ext = c->distributed();
        const bool flags = semantics == OMC_SEM_REFERENCE;
        int graphed = kNoGraph;
        if (!ext && step_graph_enabled(c)) {
            graphed = enqueue_sweep_graph(c, p, w, semantics, write_state);
            if (graphed != 0 && graphed != kNoGraph) return graphed;
        }
        if (graphed == kNoGraph) {
            const int nblk = omc::lsm_sweep_blocks(p.M);
            if (ext && p2p_active(c)) omc::p2p_begin_call(c->p2p);  // its first exchange absorbs start-up skew
            for (int t = p.N; t >= 1; --t) {
                HIP_TRY(omc::lsm_step(st, p, w, semantics, t, ext));
                if (ext && t >= 2) {
                    if (p2p_active(c)) {  // reduce + publish to all peers + gather + rank-ordered sum: one launch
                        HIP_TRY(omc::p2p_exchange_step(c->p2p, st, w, t - 1, nblk));
                        c->p2p_used = true;
                    } else {
                        HIP_TRY(omc::lsm_reduce_step_moments(st, w, t - 1, nblk));
                        if ((rc = allreduce(c, w.gmom + (size_t)(t - 1) * 8, 8))) return rc;
                    }
                }
            }
            HIP_TRY(omc::lsm_final_reduce(st, p, w, semantics == OMC_SEM_TEXTBOOK ? 0 : 1, flags, write_state));
        }
    }
    // {sum, sumsq, n_exercised, n_zero, sum_nitm, ..} -> global sums.  Slot 4 is built from the moment
    // table, which is ALREADY global on every rank: fill_result divides it by the world size again.
    // (slot 6: "a direct exchange gave up on this rank" -- after the all-reduce every rank knows, check_p2p)
    if (c->p2p_used) HIP_TRY(omc::p2p_stamp_results(c->p2p, st, w.result, 1));
    if (c->distributed() && !c->defer_result_allreduce && (rc = allreduce(c, w.result, 8))) return rc;
    return 0;
}

// ---- groups of two-pass pricings that share their small launches (omc_ctx.h)
GroupLayout::GroupLayout(int64_t M, int N)
{
    const size_t n1 = (size_t)N + 1;
    o_gmom = up256(sizeof(double) * 8 * n1 * omc::lsm_part1_tiles(M));
    o_betas = o_gmom + up256(sizeof(double) * 8 * n1);
    o_crit = o_betas + up256(sizeof(double) * 4 * n1);
    o_part = o_crit + up256(sizeof(uint32_t) * 8 * n1);
    per = o_part + up256(sizeof(double) * 2 * 8 * omc::kMaxLsmBlocks);
}

TwoPassGroup::TwoPassGroup(const GroupLayout& L_, void* state_, const omc::LsmWorkspace& w0_, bool tables_)
    : L(L_), state((char*)state_), w0(w0_), tables(tables_)
{
    g.irr_every = w0.crit_irr_every;
}

// member K (at most kSeqGroupMax) of the group: its buffers carved from the state, its slot of the argument block
void TwoPassGroup::add(const omc::LsmProblem& p, double* result)
{
    const int k = K++;
    char* st = state + L.per * (size_t)k;
    omc::LsmWorkspace& wk = w[k] = w0;
    wk.part1 = (double*)st; wk.gmom = (double*)(st + L.o_gmom); wk.betas = (double*)(st + L.o_betas);
    wk.crit = tables ? (uint32_t*)(st + L.o_crit) : nullptr; wk.part = (double*)(st + L.o_part);
    wk.result = result;
    prob[k] = p;
    g.slot[k] = omc::lsm_group_slot(p, wk);
    g.N = std::max(g.N, p.N);  // (members of one length, but for a chain's Bermudan entries: shorter)
}

// after a wait: did a direct exchange give up (its bounded poll ran out) -- on this rank (its sticky error word; the
// sums are NaN then) or on ANY rank (slot 6 of the all-reduced result sums of the n pricings just waited for)?
// Every rank of the job returns the error, not only the one whose deadline ran out.
int check_p2p(omc_ctx* c, const double* h, int n)
{
    if (!c->p2p_used) return 0;
    c->p2p_used = false;
    unsigned long long w = 0;
    HIP_TRY(omc::p2p_error_word(c->p2p, c->stream, &w));
    bool peer = false;
    for (int i = 0; h && i < n; ++i) peer = peer || h[(size_t)i * 8 + 6] != 0.0;
    if (w == 1)
        return fail(3100, "direct peer exchange of the per-step moments timed out (a peer's contribution never arrived); "
                          "omc_p2p_disconnect and use the collective");
    if (w || peer)
        return fail(3100, "direct peer exchange of the per-step moments: another rank gave up on an exchange (its deadline "
                          "ran out), so this job's sums are not to be trusted; omc_p2p_disconnect and use the collective");
    return 0;
}

void fill_result(omc_result* res, const double* h, int64_t M, int world)
{
    memset(res, 0, sizeof *res);
    res->sum = h[0];
    res->sumsq = h[1];
    res->n_paths = M;
    res->n_exercised = (int64_t)llround(h[2]);
    res->n_zero = (int64_t)llround(h[3]);
    res->sum_nitm = (int64_t)llround(h[4] / (double)world);
    res->price = h[0] / (double)M;
    const double var = h[1] / (double)M - res->price * res->price;
    res->std = var > 0 ? std::sqrt(var) : 0.0;
    res->zero_prob = (double)res->n_zero / (double)M;
}

// after a backward induction: its 8 result sums into c->hres and the caller's optional outputs, then a wait
int copy_outputs(omc_ctx* c, const omc::LsmWorkspace& w, int64_t M, int N, double* betas_out,
                 float* sx_out, int32_t* tex_out)
{
    HIP_TRY(hipMemcpyAsync(c->hres, w.result, sizeof(double) * 8, hipMemcpyDeviceToHost, c->stream));
    if (betas_out)
        HIP_TRY(hipMemcpyAsync(betas_out, w.betas, sizeof(double) * 4 * (size_t)(N + 1),
                               hipMemcpyDeviceToHost, c->stream));
    if (sx_out)
        HIP_TRY(hipMemcpyAsync(sx_out, w.sx, sizeof(float) * (size_t)M, hipMemcpyDeviceToHost, c->stream));
    if (tex_out)
        HIP_TRY(hipMemcpyAsync(tex_out, w.tex, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost,
                               c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int upload_fits(omc_ctx* c, const omc::LsmWorkspace& w, const double* betas, int N)
{
    HIP_TRY(hipMemcpyAsync(w.betas, betas, sizeof(double) * 4 * (size_t)(N + 1), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int check_heston_scheme(int scheme, double kappa, double theta, double xi)
{
    if (scheme < 0 || scheme > OMC_HESTON_QE) return fail(-4, "unknown Heston scheme.");
    if (scheme == OMC_HESTON_QE && (!(kappa > 0) || !(xi > 0) || !(theta > 0)))
        return fail(-36, "the QE scheme needs kappa, theta and xi positive.");
    return 0;
}

int check_params(const omc_params* p)
{
    int rc;
    if (!p) return fail(-7, "null params.");
    if ((rc = check_market(p->S0, p->K, p->T, p->r))) return rc;
    if ((rc = check_sizes(p->n_paths, p->n_steps))) return rc;
    if (p->model == OMC_MODEL_GBM) {
        if (!(p->sigma > 0)) return fail(-5, "S0, K, T, and sigma must be positive.");
    } else if (p->model == OMC_MODEL_HESTON) {
        if (!(p->rho >= -1.0 && p->rho <= 1.0) || !(p->v0 >= 0)) return fail(-5, "invalid Heston parameters.");
        if ((rc = check_heston_scheme(p->heston_scheme, p->kappa, p->theta, p->xi))) return rc;
        if (!p->antithetic) return fail(-4, "Heston paths are always antithetic.");
    } else {
        return fail(-4, "unknown model.");
    }
    if (p->semantics < 0 || p->semantics > 2) return fail(-4, "unknown semantics.");
    if (p->antithetic && (p->n_paths & 1)) return fail(-3, "antithetic layout needs an even n_paths.");
    return 0;
}

int check_contnet(omc_ctx* c, int hidden, int epochs, double lr)
{
    if (hidden < 1 || omc::cn_padded_width(hidden) < 0) return fail(-4, "nn_hidden must be in 1 .. 128.");
    if (epochs < 0) return fail(-4, "nn_epochs must be non-negative.");
    if (!(lr > 0.0)) return fail(-4, "nn_lr must be positive.");
    if (c->distributed()) return fail(-10, "the per-step network flow runs on one GPU.");
    return 0;
}

// ------------------------------------------------------------------ fused pricing
// `fold`: only the FIRST partner of every antithetic pair is generated (n_paths / 2 columns; the same Philox counters,
// hence the same spots, as the first half of the full matrix)
int enqueue_paths(omc_ctx* c, const omc_params* p, float* S, int64_t ld, bool fold)
{
    if (p->model == OMC_MODEL_GBM)
        HIP_TRY(omc::launch_gbm_paths(c->stream, S, ld, fold ? p->n_paths / 2 : p->n_paths, p->n_steps, p->S0, p->r,
                                      p->sigma, p->T, p->seed, (uint32_t)p->stream, p->pair_offset,
                                      fold ? 0 : p->antithetic, c->gbm_vec));
    else
        HIP_TRY(omc::launch_heston_paths(c->stream, S, ld, p->n_paths, p->n_steps, p->S0, p->r, p->T, p->v0,
                                         p->kappa, p->theta, p->xi, p->rho, p->seed, (uint32_t)p->stream,
                                         p->pair_offset, p->heston_scheme, c->heston_vec));
    return 0;
}

// How the fused pricing (the library owns the path matrix) stores the paths of `p`: antithetic GBM in the two-pass flow
// keeps only the first partner of every pair (omc_lsm_dev.h, "antithetic-folded storage") -- *cK is then table `slot` of
// S0^2 exp(2 drift t) / K, (re)filled on the stream when its inputs changed -- everything else the full matrix (*cK null).
// Small pricings stay on the full matrix: they are bound by launch latency, not by bytes (a curve point of a few thousand
// paths would pay a table refill per point for nothing), and omc_price_american_batch -- which prices such members many
// per launch on full storage -- keeps returning the bits of the single calls.  The rule looks at the JOB's paths (local
// paths x ranks), so a sharded pricing and its one-GPU form use the same storage.
constexpr int64_t kFoldMinPaths = 65536;
bool fold_applies(const omc_ctx* c, const omc_params* p)
{
    if (!c->fold || p->model != OMC_MODEL_GBM || !p->antithetic || p->semantics != OMC_SEM_TWO_PASS) return false;
    return c->fold >= 2 || p->n_paths * (int64_t)(c->world > 0 ? c->world : 1) >= kFoldMinPaths;
}

int plan_storage(omc_ctx* c, const omc_params* p, int slot, int64_t* ld, const double** cK)
{
    *cK = nullptr;
    *ld = padded_ld(p->n_paths);
    if (!fold_applies(c, p)) return 0;
    int rc;
    const size_t per = (size_t)omc::kMaxSteps + 2;
    if ((rc = c->foldC.ensure(sizeof(double) * 2 * per))) return rc;
    double* tab = (double*)c->foldC.p + per * (size_t)slot;
    double c0, g;
    omc::gbm_fold_constants(p->S0, p->K, p->r, p->sigma, p->T, p->n_steps, &c0, &g);
    omc_ctx::FoldKey& key = c->fold_key[slot];
    if (key.N != p->n_steps || key.c0 != c0 || key.g != g) {
        HIP_TRY(omc::lsm_fold_table(c->stream, tab, p->n_steps, c0, g));
        key.N = p->n_steps; key.c0 = c0; key.g = g;
    }
    *ld = padded_ld(p->n_paths / 2);
    *cK = tab;
    return 0;
}

// The context's own path matrix c->S for `p`, stored as plan_storage decides (cK table 0) or, for the flows that read
// every path of it (barrier, ols7, ContNet), always in full.
int ensure_paths(omc_ctx* c, const omc_params* p, Storage how, float** S, int64_t* ld, const double** cK)
{
    int rc;
    if (how == Storage::planned && (rc = plan_storage(c, p, 0, ld, cK))) return rc;
    if (how == Storage::full_only) *ld = padded_ld(p->n_paths);
    if ((rc = c->S.ensure(sizeof(float) * (size_t)*ld * (size_t)(p->n_steps + 1)))) return rc;
    *S = (float*)c->S.p;
    return 0;
}

// Enqueue one whole pricing (paths + backward induction) on the context's stream; its 8 result sums
// go to `result_dev` (device-visible memory) or, when null, to the workspace's device buffer, which is
// returned through *result_out.  Events are recorded only when `timed`.  `gen` (null: p itself) holds the parameters of
// the generator / fold-table side: p with the drift rate of the paths where that is not the discount rate.
int enqueue_pricing(omc_ctx* c, const omc_params* p, float* S_keep, int64_t ld, double* result_dev,
                    hipEvent_t* evs, double** result_out, const omc_params* gen)
{
    if (!gen) gen = p;
    const bool timed = evs != nullptr;
    int rc;
    const int64_t M = p->n_paths;
    const int N = p->n_steps;
    float* S = S_keep;
    const double* cK = nullptr;
    if (S) {
        if (ld < M) return fail(-6, "leading dimension smaller than n_paths.");
    } else if ((rc = ensure_paths(c, gen, Storage::planned, &S, &ld, &cK))) {
        return rc;
    }
    omc::LsmWorkspace w;
    if ((rc = prepare_lsm(c, M, N, p->r, p->T, p->semantics == OMC_SEM_TWO_PASS, false, &w))) return rc;
    omc::LsmProblem prob{S, ld, M, N, p->is_put ? 1 : 0, p->K, p->r, p->T};
    prob.fold_cK = cK;
    if (timed) {
        // (pass 1 starts where the generator ends: evs[1] is its begin; an event costs ~3 us of dispatch gap)
        w.ev_p1_end = evs[4]; w.ev_p2_begin = evs[5]; w.ev_p2_end = evs[6];
        HIP_TRY(hipEventRecord(evs[0], c->stream));
    }
    if ((rc = enqueue_paths(c, gen, S, ld, cK != nullptr))) return rc;
    if (timed) HIP_TRY(hipEventRecord(evs[1], c->stream));
    if (result_dev) w.result = result_dev;
    if ((rc = enqueue_lsm(c, prob, w, p->semantics, false))) return rc;
    if (result_out) *result_out = w.result;
    return 0;
}

// omc_price_american behind its argument checks: one timed pricing on the context's stream and its result (gen: as
// enqueue_pricing)
int price_fused(omc_ctx* c, const omc_params* p, const omc_params* gen, omc_result* res, float* S_keep, int64_t ld)
{
    int rc;
    // Single GPU: the finalize kernel stores its 8 sums straight into host-mapped pinned memory (no copy
    // kernel, no extra dependent launch).  With an all-reduce hook the sums stay in device memory for
    // the collective and are copied afterwards.
    const bool zero_copy = c->hres_dev && !c->distributed();
    double* hres = c->hres_pin ? c->hres_pin : c->hres;
    double* result = nullptr;
    if ((rc = enqueue_pricing(c, p, S_keep, ld, zero_copy ? c->hres_dev : nullptr, c->ev, &result, gen))) return rc;
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    if (!zero_copy)
        HIP_TRY(hipMemcpyAsync(hres, result, sizeof(double) * 8, hipMemcpyDeviceToHost, c->stream));
    if ((rc = wait_stream(c))) return rc;
    if ((rc = check_p2p(c, hres, 1))) return rc;
    fill_result(res, hres, c->distributed() ? p->n_paths * c->world : p->n_paths,
                c->distributed() ? c->world : 1);  // distributed: sums are global
    res->folded = (!S_keep && fold_applies(c, p)) ? 1 : 0;
    return read_kernel_times(c->ev, p, res);
}

// HIP-event times of a pricing with enqueue_pricing's events: evs[0] paths evs[1] backward induction evs[2] (when
// `has_end`); for a two-pass pricing `p` of two steps or more also pass 1 (evs[1] .. evs[4]) and pass 2 (evs[5] .. evs[6]).
// p == nullptr: no pass times.
int read_kernel_times(const hipEvent_t* evs, const omc_params* p, omc_result* res, bool has_end)
{
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, evs[0], evs[1]));
    res->ms_paths = ms;
    if (has_end) {
        HIP_TRY(hipEventElapsedTime(&ms, evs[1], evs[2]));
        res->ms_lsm = ms;
        res->ms_total = res->ms_paths + res->ms_lsm;
    }
    if (p && p->semantics == OMC_SEM_TWO_PASS && p->n_steps >= 2) {
        HIP_TRY(hipEventElapsedTime(&ms, evs[1], evs[4]));
        res->ms_pass1 = ms;
        HIP_TRY(hipEventElapsedTime(&ms, evs[5], evs[6]));
        res->ms_pass2 = ms;
    }
    return 0;
}

// ------------------------------------------------------------------ generate, then the two-pass sweeps
omc::PathSpec path_spec(const omc_ctx* c, const omc_params* p, double drift_rate, float* S, int64_t ld)
{
    omc::PathSpec g{};
    g.model = p->model == OMC_MODEL_GBM ? 0 : 1; g.scheme = p->heston_scheme;
    g.n_paths = p->n_paths; g.n_steps = p->n_steps;
    g.S0 = p->S0; g.r = drift_rate; g.sigma = p->sigma; g.T = p->T;
    g.v0 = p->v0; g.kappa = p->kappa; g.theta = p->theta; g.xi = p->xi; g.rho = p->rho;
    g.seed = p->seed; g.pair_offset = p->pair_offset; g.stream = (uint32_t)p->stream;
    g.vec_hint = g.model == 0 ? c->gbm_vec : c->heston_vec;
    g.S = S; g.ld = ld;
    return g;
}

omc::PathSpec path_spec(const omc_ctx* c, const omc_params* p, double drift_rate, float* S, int64_t ld, int64_t n_paths,
                        uint64_t stream, uint64_t pair_offset)
{
    omc::PathSpec g = path_spec(c, p, drift_rate, S, ld);
    g.n_paths = n_paths; g.stream = (uint32_t)stream; g.pair_offset = pair_offset;
    return g;
}

int take_full_matrix(omc_ctx* c, const omc_params* p, float* S_keep, float** S, int64_t* ld)
{
    if (S_keep && *ld < p->n_paths) return fail(-6, "leading dimension smaller than n_paths.");
    *S = S_keep;
    return S_keep ? 0 : ensure_paths(c, p, Storage::full_only, S, ld);
}

int enqueue_generated(omc_ctx* c, const omc_params* p, const float* S, int64_t ld,
                      const std::function<hipError_t(hipStream_t)>& gen)
{
    int rc;
    omc::LsmWorkspace w;
    if ((rc = prepare_lsm(c, p->n_paths, p->n_steps, p->r, p->T, true, false, &w))) return rc;
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    HIP_TRY(gen(c->stream));
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    omc::LsmProblem prob{S, ld, p->n_paths, p->n_steps, p->is_put ? 1 : 0, p->K, p->r, p->T};
    w.ev_p1_end = c->ev[4]; w.ev_p2_begin = c->ev[5]; w.ev_p2_end = c->ev[6];
    if ((rc = enqueue_lsm(c, prob, w, OMC_SEM_TWO_PASS, false))) return rc;
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    HIP_TRY(hipMemcpyAsync(c->hres, w.result, sizeof(double) * 8, hipMemcpyDeviceToHost, c->stream));
    return 0;
}

int finish_generated(omc_ctx* c, const omc_params* p, omc_result* base)
{
    int rc;
    if ((rc = wait_stream(c))) return rc;
    fill_result(base, c->hres, p->n_paths);
    base->folded = 0;
    return read_kernel_times(c->ev, p, base);
}

}  // namespace omc::abi

using namespace omc::abi;

// Everything the context holds that is not a member with a destructor of its own (the DevBufs free themselves after
// this); the caller has made the context's device current.
omc_ctx::~omc_ctx()
{
    drop_sweep_graph(this);
    if (comm) omc::comm_destroy(comm);
    if (p2p) omc::p2p_destroy(p2p);
    if (hres_pin) (void)hipHostFree(hres_pin);
    if (seq_pin) (void)hipHostFree(seq_pin);
    if (sweep_pin) (void)hipHostFree(sweep_pin);
    if (mtab_pin) (void)hipHostFree(mtab_pin);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_pool) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {ev_seq, ev_entry, ev_moments[0], ev_moments[1], ev_reduced[0], ev_reduced[1]})
        if (e) (void)hipEventDestroy(e);
    if (comm_stream) (void)hipStreamDestroy(comm_stream);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
}

extern "C" {

int omc_abi_version(void) { return OMC_ABI_VERSION; }

const char* omc_last_error(void) { return g_err.c_str(); }

int omc_device_count(int* count)
{
    if (!count) return fail(-7, "null pointer.");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        (void)hipGetLastError();
        g_err = std::string("hipGetDeviceCount: ") + hipGetErrorString(e);
        return (int)e;
    }
    *count = n;
    return 0;
}

int omc_ctx_create(int device, void* hip_stream, omc_ctx** out)
{
    if (!out) return fail(-7, "null pointer.");
    *out = nullptr;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(-4, "no such HIP device.");
    HIP_TRY(hipSetDevice(device));
    omc_ctx* c = new omc_ctx();
    c->device = device;
    auto undo = [&](hipError_t e) { delete c; return e; };  // release what was created so far, report e
    if (hip_stream) {
        c->stream = (hipStream_t)hip_stream;
        c->own_stream = false;
    } else {
        const hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            c->stream = nullptr;
            HIP_TRY(undo(e));
        }
        c->own_stream = true;
    }
    for (auto& ev : c->ev) {
        const hipError_t e = hipEventCreate(&ev);
        if (e != hipSuccess) {
            ev = nullptr;
            HIP_TRY(undo(e));
        }
    }
    if (hipHostMalloc((void**)&c->hres_pin, sizeof(double) * 8, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&c->hres_dev, c->hres_pin, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (c->hres_pin) (void)hipHostFree(c->hres_pin);
        c->hres_pin = c->hres_dev = nullptr;  // fall back to a device buffer + copy into the pageable member
    }
    (void)hipDeviceGetAttribute(&c->device_cus, hipDeviceAttributeMultiprocessorCount, device);
    *out = c;
    return 0;
}

int omc_ctx_destroy(omc_ctx* c)
{
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    delete c;
    return 0;
}

int omc_ctx_device_info(omc_ctx* c, int* device, char* pci_bus_id, int pci_len, char* name, int name_len)
{
    int rc = bind(c);
    if (rc) return rc;
    if (device) *device = c->device;
    if (pci_bus_id && pci_len > 0) {
        pci_bus_id[0] = 0;
        HIP_TRY(hipDeviceGetPCIBusId(pci_bus_id, pci_len, c->device));
    }
    if (name && name_len > 0) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, c->device));
        snprintf(name, (size_t)name_len, "%s", prop.name);
    }
    return 0;
}

int omc_sync(omc_ctx* c)
{
    int rc = bind(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int omc_alloc(omc_ctx* c, size_t bytes, void** dptr)
{
    int rc = bind(c);
    if (rc) return rc;
    if (!dptr) return fail(-7, "null pointer.");
    HIP_TRY(hipMalloc(dptr, bytes ? bytes : 1));
    return 0;
}

int omc_free(omc_ctx* c, void* dptr)
{
    int rc = bind_in(c);
    if (rc) return rc;
    if (dptr) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipFree(dptr));
    }
    return 0;
}

static int copy_and_wait(omc_ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind)
{
    int rc = bind_in(c);
    if (rc) return rc;
    if (!bytes) return 0;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int omc_memcpy_h2d(omc_ctx* c, void* dst, const void* src, size_t bytes)
{
    return copy_and_wait(c, dst, src, bytes, hipMemcpyHostToDevice);
}

int omc_memcpy_d2h(omc_ctx* c, void* dst, const void* src, size_t bytes)
{
    return copy_and_wait(c, dst, src, bytes, hipMemcpyDeviceToHost);
}

int omc_set_option(omc_ctx* c, const char* key, int64_t value)
{
    if (!c || !key) return fail(-7, "null pointer.");
    if (!strcmp(key, "gbm_vec")) c->gbm_vec = (int)value;
    else if (!strcmp(key, "alloc_limit")) g_alloc_limit = value > 0 ? (size_t)value : 0;
    else if (!strcmp(key, "fold_antithetic")) c->fold = value <= 0 ? 0 : (value >= 2 ? 2 : 1);
    else if (!strcmp(key, "pass2_tables")) c->pass2_tables = value ? 1 : 0;
    else if (!strcmp(key, "pass2_tables_irregular_every")) c->pass2_irr_every = value > 0 ? (int)value : 0;
    else if (!strcmp(key, "heston_vec")) c->heston_vec = (int)value;
    else if (!strcmp(key, "world_size")) c->world = value > 0 ? (int)value : 1;
    else if (!strcmp(key, "step_graph")) c->step_graph = value < 0 ? -1 : (value ? 1 : 0);
    else if (!strcmp(key, "seq_overlap")) c->seq_overlap = value < 0 ? -1 : (value ? 1 : 0);
    else if (!strcmp(key, "seq_event_stride")) c->seq_event_stride = value > 0 ? (int)value : 0;
    else if (!strcmp(key, "seq_step_k")) c->seq_step_k = value < 0 ? -1 : (int)(value > 32 ? 32 : value);
    else if (!strcmp(key, "seq_two_pass_k")) c->seq_two_pass_k = value < 0 ? -1 : (int)(value > 32 ? 32 : value);
    else if (!strcmp(key, "bounds_exercise_every")) {
        if (value < 0 || value > 2147483647) return fail(-4, "bounds_exercise_every must be in 0 .. 2^31 - 1.");
        c->bounds_every = value;
    }
    else if (!strcmp(key, "bounds_control_variate")) {
        if (value != 0 && value != 1) return fail(-4, "bounds_control_variate must be 0 or 1.");
        c->bounds_cv = (int)value;
    }
    else if (!strcmp(key, "bounds_cv_form")) {
        if (value != 0 && value != 1) return fail(-4, "bounds_cv_form must be 0 or 1.");
        c->bounds_cv_form = (int)value;
    }
    else if (!strcmp(key, "bounds_suboptimality")) {
        if (value < 0 || value > 2) return fail(-4, "bounds_suboptimality must be 0 (off), 1 (payoff) or 2 (European).");
        c->bounds_subopt = (int)value;
    }
    else if (!strcmp(key, "chain_fused")) c->chain_fused = value ? 1 : 0;
    else if (!strcmp(key, "chain_k")) c->chain_k = value < 1 ? -1 : (int)(value > 16 ? 16 : value);
    else if (!strcmp(key, "chain_greeks_k")) {
        if (value != -1 && (value < 1 || value > 16)) return fail(-4, "chain_greeks_k must be -1 (default) or 1 .. 16.");
        c->chain_greeks_k = (int)value;
    }
    else if (!strcmp(key, "chain_greeks_order")) {
        if (value != 0 && value != 1) return fail(-4, "chain_greeks_order must be 0 (banded) or 1 (plain).");
        c->chain_greeks_order = (int)value;
    }
    else if (!strcmp(key, "seq_step_wgs")) c->seq_step_wgs = value > 0 ? (int)value : 0;
    else if (!strcmp(key, "p2p_exchange")) c->p2p_use = value ? 1 : 0;
    else if (!strcmp(key, "p2p_deadline_ms") || !strcmp(key, "p2p_first_deadline_ms")) {
        if (value <= 0) return fail(-4, "a p2p deadline must be positive.");
        (key[4] == 'f' ? c->p2p_first_deadline_s : c->p2p_deadline_s) = (double)value * 1e-3;
        if (c->p2p) omc::p2p_set_deadline(c->p2p, c->p2p_deadline_s, c->p2p_first_deadline_s);
    }
    else return fail(-4, "unknown option key.");
    return 0;
}

int omc_set_allreduce_hook(omc_ctx* c, omc_allreduce_fn fn, void* user)
{
    if (!c) return fail(-7, "null context.");
    if (fn) {
        // the few hundred bytes every collective vote / flag exchange goes through: allocated HERE, so that no allocation
        // -- nothing that can fail on one rank alone -- stands between a rank and a collective its peers have entered
        int rc;
        if ((rc = bind(c))) return rc;
        if ((rc = c->seq_vote.ensure(kVoteBytes))) return rc;
    }
    c->hook = fn;
    c->hook_user = user;
    return 0;
}

// ------------------------------------------------------------------ native RCCL communicator
int omc_comm_unique_id(void* uid_out, size_t bytes)
{
    if (!uid_out || bytes < (size_t)omc::kCommUidBytes) return fail(-7, "unique-id buffer must hold 128 bytes.");
    std::string err;
    const int rc = omc::comm_unique_id(uid_out, &err);
    if (rc) return fail(rc, err.c_str());
    return 0;
}

int omc_comm_init(omc_ctx* c, int rank, int world, const void* uid, size_t bytes)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!uid || bytes < (size_t)omc::kCommUidBytes) return fail(-7, "unique id must be 128 bytes.");
    if (world < 1 || rank < 0 || rank >= world) return fail(-4, "rank / world size out of range.");
    if (c->comm) return fail(-4, "this context already has a communicator.");
    std::string err;
    omc::Comm* comm = nullptr;
    if ((rc = c->seq_vote.ensure(kVoteBytes))) return rc;  // (see omc_set_allreduce_hook; before the collective bring-up)
    rc = omc::comm_create(rank, world, uid, &comm, &err);
    if (rc) return fail(rc, err.c_str());
    c->comm = comm;
    c->world = omc::comm_world(comm);
    return 0;
}

int omc_comm_destroy(omc_ctx* c)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!c->comm) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    omc::comm_destroy(c->comm);
    c->comm = nullptr;
    c->world = 1;
    return 0;
}

int omc_comm_info(omc_ctx* c, int* rank, int* world)
{
    if (!c) return fail(-7, "null context.");
    if (rank) *rank = omc::comm_rank(c->comm);
    if (world) *world = c->comm ? omc::comm_world(c->comm) : 0;
    return 0;
}

int omc_comm_allreduce_f64(omc_ctx* c, double* host_inout, int count, int op)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!c->comm) return fail(-4, "no communicator on this context (omc_comm_init).");
    if (!host_inout || count <= 0 || count > 4096) return fail(-7, "bad buffer (1..4096 doubles).");
    if (op != 0 && op != 1) return fail(-4, "op must be 0 (sum) or 1 (max).");
    if ((rc = c->scratch.ensure(sizeof(double) * 4096))) return rc;
    double* d = (double*)c->scratch.p;
    HIP_TRY(hipMemcpyAsync(d, host_inout, sizeof(double) * (size_t)count, hipMemcpyHostToDevice, c->stream));
    std::string err;
    rc = omc::comm_allreduce_f64(c->comm, d, (size_t)count, op, c->stream, &err);
    if (rc) return fail(rc, err.c_str());
    HIP_TRY(hipMemcpyAsync(host_inout, d, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// ------------------------------------------------------------------ direct peer exchange (per-step flows)
int omc_p2p_export(omc_ctx* c, void* handle_out, size_t bytes)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!handle_out || bytes < (size_t)omc::kP2PHandleBytes) return fail(-7, "handle buffer must hold 64 bytes.");
    if (c->p2p) return fail(-4, "this context already has a mailbox (omc_p2p_disconnect first).");
    std::string err;
    omc::P2P* p = nullptr;
    rc = omc::p2p_export(&p, handle_out, &err);
    if (rc) return fail(rc, err.c_str());
    c->p2p = p;
    omc::p2p_set_deadline(p, c->p2p_deadline_s, c->p2p_first_deadline_s);
    return 0;
}

int omc_p2p_connect(omc_ctx* c, int rank, int world, const void* handles, size_t bytes)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!c->p2p) return fail(-4, "no mailbox on this context (omc_p2p_export first).");
    if (!handles || world < 1 || bytes < (size_t)world * omc::kP2PHandleBytes)
        return fail(-7, "handles must hold world x 64 bytes, in rank order.");
    std::string err;
    rc = omc::p2p_connect(c->p2p, rank, world, handles, &err);
    if (rc) return fail(rc, err.c_str());
    return 0;
}

int omc_p2p_disconnect(omc_ctx* c)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!c->p2p) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    omc::p2p_destroy(c->p2p);
    c->p2p = nullptr;
    c->p2p_used = false;
    return 0;
}

int omc_p2p_status(omc_ctx* c, int* connected, int* world, uint64_t* error_word)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (connected) *connected = (c->p2p && omc::p2p_connected(c->p2p)) ? 1 : 0;
    if (world) *world = c->p2p ? omc::p2p_world(c->p2p) : 0;
    if (error_word) {
        *error_word = 0;
        if (c->p2p && omc::p2p_connected(c->p2p)) {
            unsigned long long w = 0;
            HIP_TRY(omc::p2p_error_word(c->p2p, c->stream, &w));
            *error_word = w;
        }
    }
    return 0;
}

}  // extern "C"
