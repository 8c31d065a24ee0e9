/*
 * omc.h -- C ABI of libomc.so: MI355X (gfx950) American-option Monte-Carlo hot path.
 *
 * The reference (Levicoz/Options-model) is 100 % Python and has no FFI, plugin or operator
 * interface; its boundary for this path is the Python call surface.  This header is the
 * drop-in boundary underneath that surface: each entry point names the reference code it
 * replaces (paths relative to the reference root).  Host bindings: ctypes, see
 * options_model_amd/_ffi.py and INTEGRATION.md.
 *
 * Conventions
 *   - every function returns int: 0 ok; <0 invalid argument (Python raises ValueError with
 *     the reference's message); >0 a hipError_t (Python raises RuntimeError).
 *     omc_last_error() returns a thread-local description of the last failure.
 *   - no HIP call happens at load time; a context is created lazily per (process, device),
 *     so the library is safe under the reference's `spawn`ed ProcessPoolExecutor workers
 *     (options_model_2_ui.py:8-11).
 *   - path matrices are float32 [n_steps+1][ld], row = time step, ld >= n_paths elements
 *     (the reference's S[t, j] C-order layout, options_model_3/options_model_3.py:477).
 *     Antithetic partner of column j is j + n_paths/2 (options_model_3.py:476).
 *   - device pointers passed in are borrowed; the library frees only what omc_alloc returned.
 *   - calls on one context are serialised by the caller; all entry points are synchronous
 *     (return after the stream has drained) unless stated otherwise.
 */
#ifndef OMC_H
#define OMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OMC_ABI_VERSION 14

typedef struct omc_ctx omc_ctx;

/* semantics of the backward induction */
enum {
    OMC_SEM_REFERENCE = 0, /* per-step sticky flow: Options_model.py:108-157, options_model_2.py:278-313 */
    OMC_SEM_TEXTBOOK = 1,  /* classic Longstaff-Schwartz, discounted to t=0                        */
    OMC_SEM_TWO_PASS = 2   /* v3 flow: options_model_3/options_model_3.py:482-516 + :615-651        */
};
enum { OMC_MODEL_GBM = 0, OMC_MODEL_HESTON = 1 };
enum {
    OMC_HESTON_REFERENCE_CLAMP = 0, /* options_model_3.py:230-233                                 */
    OMC_HESTON_FULL_TRUNCATION = 1, /* Lord et al. (named by BASELINE.json)                       */
    OMC_HESTON_CALIBRATOR = 2,      /* heston_calibration.py:242-255: floor 1e-8, arithmetic Euler */
    OMC_HESTON_QE = 3               /* Andersen (2008) quadratic-exponential; the rule is below    */
};
/* OMC_HESTON_QE -- the step of one antithetic pair.  Needs kappa > 0, theta > 0, xi > 0: every entry
 * point that takes a Heston scheme refuses it otherwise with -36 before anything is launched (-4 stays "unknown scheme").
 * Taken wherever a scheme is taken except the price bounds (omc_price_american_bounds_heston: -12).  No struct layout and
 * no OMC_ABI_VERSION change: heston_scheme had the room.
 *   Constants, formed in double and rounded to float32 once (dt = T / n_steps, E = exp(-kappa dt), L = log2 e):
 *     c1 = xi^2 E (1 - E) / kappa,  c2 = theta xi^2 (1 - E)^2 / (2 kappa),
 *     k0 = L (r dt - rho kappa theta dt / xi),  k1 = L (dt (kappa rho / xi - 1/2) / 2 - rho / xi),
 *     k2 = L (dt (kappa rho / xi - 1/2) / 2 + rho / xi),  k34 = L^2 dt (1 - rho^2) / 2      (gamma1 = gamma2 = 1/2).
 *   Draws: Zv = z1, Zs = z2 of the pair's Philox block, two steps per block as for the Euler schemes; the partner takes
 *     (-Zv, -Zs).  No further random words.
 *   float32 state (s, v), v >= 0, in this order (fma = one rounding; rcp, sqrt, exp2 the hardware's ~1 ulp instructions):
 *     m = fma(v - theta, E, theta);  s2 = fma(v, c1, c2);  m2 = m m;   psi = s2 / m2 is > 1.5 iff s2 > 1.5f m2
 *     psi <= 1.5:  t = (m2 + m2) rcp(s2)  [= 2 / psi];  b2 = (t - 1) + sqrt(t (t - 1));  a = m rcp(1 + b2);
 *                  v' = a (sqrt(b2) + Zv)^2
 *     psi > 1.5:   q = fma(s2, rcp(m2), 1)  [= psi + 1];  1 - p = 2 / q;  Q = erfcf(Zv / sqrt 2) / 2  (the UPPER tail, 1 - U
 *                  with U = Phi(Zv), formed directly: the partner's is erfcf(-Zv / sqrt 2) / 2, not a subtraction);
 *                  v' = max(0, (logf(1 - p) - logf(Q)) (m q / 2))            [1 / beta = m / (1 - p) = m q / 2]
 *     s' = s exp2(fma(sqrt(fma(k34, v', k34 v)), Zs, fma(k2, v', fma(k1, v, k0))))
 *   No martingale correction (K0*), no floor in the arithmetic.  omc_heston_paths_sv_f32 stores v' (row t, after step t). */

typedef struct {
    int32_t model;         /* OMC_MODEL_*                                               */
    int32_t is_put;        /* payoff: options_model_3.py:376-380                          */
    int32_t semantics;     /* OMC_SEM_*                                                 */
    int32_t antithetic;    /* 1 = reference layout (GBM only may pass 0)                */
    int32_t heston_scheme; /* OMC_HESTON_*                                              */
    int32_t n_steps;
    int64_t n_paths;       /* LOCAL paths of this context (even when antithetic)        */
    double S0, K, r, sigma, T;
    double v0, kappa, theta, xi, rho; /* Heston only (dict keys of options_model_2_ui.py:74-80) */
    uint64_t seed;         /* Philox key                                                */
    uint64_t stream;       /* sub-stream id (low 32 bits used): one per pricing call    */
    uint64_t pair_offset;  /* global index of this context's first pair (multi-GPU)     */
} omc_params;

typedef struct {
    double price;          /* mean cash-flow (reference flows: valued at t = dt)   */
    double sum, sumsq;     /* over the local paths                                        */
    double std;            /* population std, as Options_model.py:154                     */
    double zero_prob;      /* P(cash-flow == 0), Options_model.py:155                     */
    int64_t n_paths, n_exercised, n_zero, sum_nitm;
    double ms_paths, ms_lsm, ms_total; /* HIP-event times of this call on the context's stream */
    double ms_pass1, ms_pass2;         /* omc_price_american, two-pass flow: the two big LSM kernels (ms_pass2: with the
                                          table build in front of the sweep; the sweep alone for a member of a group of
                                          omc_price_american_seq, see omc_seq_group_width) */
    int64_t timed;         /* omc_price_american_seq: 1 = this pricing carried its own HIP events (the ms_* kernel
                              times above are its own), 0 = they repeat those of the latest timed pricing before it */
    int64_t folded;        /* omc_price_american (no S_keep) / _seq: 1 = the pricing ran on antithetic-FOLDED storage
                              (option "fold_antithetic", below): only the first partner of every pair was stored */
} omc_result;

/* ---- library / context --------------------------------------------------------------- */
int omc_abi_version(void);
const char* omc_last_error(void);
int omc_device_count(int* count);
/* Which card a context runs on: its HIP ordinal in this process, its PCI bus id ("0000:c1:00.0", at least 13 bytes + NUL)
 * and its name.  A multi-rank job gathers these to prove that N ranks sit on N DISTINCT cards (bench.py --gpus N fails
 * loudly otherwise).  Any of the output pointers may be NULL. */
int omc_ctx_device_info(omc_ctx* ctx, int* device, char* pci_bus_id, int pci_len, char* name, int name_len);
/* hip_stream == NULL: the context creates its own stream; else it borrows the caller's
 * (e.g. torch.cuda.current_stream().cuda_stream) and never destroys it.
 *
 * Stream ordering of borrowed device pointers (the entry/exit contract):
 *   exit   every entry point returns after the context's stream has drained, so whatever the caller
 *          enqueues afterwards, on any stream, sees the library's writes.
 *   entry  a context that BORROWS a stream is ordered by that stream: the caller's pending work on it
 *          precedes the library's.  A context that OWNS its stream (hip_stream == NULL; created with
 *          hipStreamNonBlocking, so the null stream's implicit synchronisation does not apply to it) orders
 *          itself, on entry of every call that takes a device pointer from the caller, after everything then
 *          pending on the device's DEFAULT (null) stream -- the stream PyTorch queues on unless told otherwise
 *          -- by an event wait; no host blocking.  Work the caller has pending on any OTHER stream (a torch
 *          side stream, its own non-blocking streams) is not ordered: synchronise that stream first, or create
 *          the context on it.  The options_model_amd modules that hand torch tensors to the library create their
 *          contexts on torch's current stream (nn_regressor._ctx_on_torch_stream). */
int omc_ctx_create(int device, void* hip_stream, omc_ctx** out);
int omc_ctx_destroy(omc_ctx* ctx);
int omc_sync(omc_ctx* ctx);
int omc_alloc(omc_ctx* ctx, size_t bytes, void** dptr);
int omc_free(omc_ctx* ctx, void* dptr);
int omc_memcpy_h2d(omc_ctx* ctx, void* dst, const void* src, size_t bytes);
int omc_memcpy_d2h(omc_ctx* ctx, void* dst, const void* src, size_t bytes);
/* knobs: "fold_antithetic" (1 = default: the fused pricing calls -- omc_price_american without S_keep and
 * omc_price_american_seq -- keep antithetic GBM paths of the two-pass flow in FOLDED storage when the pricing has at least
 * 65,536 paths over all ranks (smaller ones are launch-bound and stay on the full matrix, bit-equal to their
 * omc_price_american_batch form); 2 = whatever the size; 0 = never.  Folded storage: since S_t S'_t = S0^2
 * exp(2 drift t) for the partners of a pair, only the first partner's path is generated and stored, half the matrix, and
 * both sweeps price the partner from the same spot through its moneyness (C_t / K) / S_t - 1 in float64 -- same Philox
 * normals, same first partners bit for bit, partner spots equal to the stored float32 ones up to their rounding (prices
 * agree to ~1e-6 relative; omc_result.folded says which storage a pricing used; oracle: orc_lsm_two_pass_folded).
 * Full storage = both partners, the layout omc_gbm_paths + omc_lsm produce),
 * "pass2_tables" (1 = default: pass 2 of the two-pass flow on folded storage decides from per-step float32 exercise tables,
 * the spot bit patterns at which its float64 decision switches, built by one small kernel right before the sweep; 0 = the
 * float64 decisions per spot; both give the same decisions, so the same results bit for bit),
 * "pass2_tables_irregular_every" (tests: k > 0 marks every k-th step of the tables irregular, i.e. decided by the float64
 * fallback inside the table sweep; 0 = default, none),
 * "gbm_vec" / "heston_vec" (pairs per thread: 1,2,4; 0 = auto), "world_size" (ranks behind
 * the all-reduce hook, see below), "step_graph" (1 / 0: replay the per-step sweep as one captured HIP
 * graph or launch its kernels one by one; -1 = default, off: same speed at 1M x 252, and a capture per new
 * geometry costs milliseconds), "seq_overlap" (omc_price_american_seq on a context with a communicator, two-pass flow, equal geometry:
 * 1 = the moment all-reduce of pricing k runs on a second stream under the path generation of pricing k+1
 * (second path buffer) and all result sums travel in one collective at the end -- bit-identical results;
 * 0 = one pricing after the other; -1 = default: off -- a job turns it on after it has checked, on its live
 * communicator, that both forms return the same bits, as bench.py does),
 * "seq_event_stride" (omc_price_american_seq: k > 0 = every k-th pricing of a sequence carries its own HIP
 * events, so a sequence yields several samples of the per-kernel times; 0 = default: the first pricing only),
 * "seq_step_k" / "seq_two_pass_k" (omc_price_american_seq: pricings per shared launch of the per-step flows / per group
 * of the two-pass flow; see omc_seq_step_width and omc_seq_group_width),
 * "chain_fused" / "chain_k" (omc_price_american_chain: 1 / 0 (default) = the fused chain sweeps or the single-strike sweeps per
 * entry; entries per fused launch, -1 = default, 1 .. 16; see omc_chain_width),
 * "bounds_exercise_every" (omc_price_american_bounds and omc_price_american_bounds_heston with a policy on the spot: 0 =
 * default or 1 = the game with exercise at every date of the grid; k >= 2 = the game with exercise at every k-th date
 * counted back from expiry, and at expiry, on paths of the whole grid -- it changes the GAME whose value is bounded, not
 * the route by which the same numbers are computed; see "an exercise schedule" in the price bounds section.  k < 0 or
 * k > 2^31 - 1 is refused with -4 and the stored value stays; the other three bounds calls refuse k >= 2 with -38),
 * "bounds_control_variate" (omc_price_american_bounds: 0 = default, 1 = the discounted Black-Scholes value of the European
 * option as a control variate in the lower bound and in every inner mean -- the same paths and stops, far smaller standard
 * errors; see "the Black-Scholes control variate" in the price bounds section.  Another value is refused with -4 and the
 * stored value stays; the other bounds calls refuse 1 with -39),
 * "bounds_suboptimality" (the price bounds on one float32 index -- omc_price_american_bounds, omc_price_american_basket_bounds
 * with the policy on the index, omc_price_american_bounds_heston with regressors spot: 0 = default, 1 = "payoff", 2 =
 * "European", omc_price_american_bounds only: Broadie-Cao's sub-optimality checking -- inner simulations only at the (outer
 * path, date) items at which exercise is not known to be sub-optimal, the same lower bound, an upper bound that can only
 * fall and stays one; see "sub-optimality checking" in the price bounds section.  Another value is refused with -4 and the
 * stored value stays; a bounds call that does not take the value is refused with -40),
 * "alloc_limit" (PER PROCESS, bytes; 0 = none: no single buffer of the library -- path matrix, workspace, row scratch --
 * may grow beyond it; a larger request fails like a hipMalloc that found no room, code 2 = hipErrorOutOfMemory.  A
 * budget for a card shared with other tenants; on a distributed context such a rank-local failure is reported on
 * EVERY rank, see "failures only one rank can see" below) */
int omc_set_option(omc_ctx* ctx, const char* key, int64_t value);
/* ---- per-step flows across GPUs without a collective per step ------------------------------ */
/* The per-step flows exchange 8 doubles per pricing after every time step.  Instead of an all-reduce per step, every
 * rank can WRITE its contribution into every peer's memory (xGMI) and sum what arrives itself: omc_p2p_export
 * allocates this rank's mailbox (fine-grained device memory) and returns its 64-byte IPC handle; hand all ranks'
 * handles, in rank order, to omc_p2p_connect on every rank (one node; at most 16 ranks).  From then on a context
 * that is distributed (communicator or hook) runs the per-step exchange as ONE small launch per step -- reduce the
 * rank's partials, publish to all peers, poll the own mailbox (bounded), add the contributions in rank order -- and
 * keeps the collective for everything else (the two-pass flow's moment table, the result sums).  Every rank gets
 * the same bits; a contribution that does not arrive within the deadline makes the pricing call fail (error 3100,
 * sticky: omc_p2p_status reports it) -- it never hangs.  Option "p2p_exchange" = 0 switches back to the collective
 * without disconnecting; "p2p_deadline_ms" = how long an exchange waits for a peer's contribution (default 2000),
 * "p2p_first_deadline_ms" = the same for the FIRST exchange of a pricing call (default 30000: nothing aligns the ranks
 * before it, and a first-use code-object load or a multi-GB allocation on one rank can skew them by seconds).
 * The failure is COLLECTIVE: a rank that gave up poisons its slot in every peer's mailbox and adds its error word to
 * the all-reduced result sums, so every rank of the job returns 3100 -- a peer that was merely slow cannot leave the
 * others with a finite price built on a contribution that was given up on.  */
int omc_p2p_export(omc_ctx* ctx, void* handle_out, size_t bytes /* >= 64 */);
int omc_p2p_connect(omc_ctx* ctx, int rank, int world, const void* handles, size_t bytes /* >= world * 64 */);
int omc_p2p_disconnect(omc_ctx* ctx);
int omc_p2p_status(omc_ctx* ctx, int* connected, int* world, uint64_t* error_word);

/* ---- path generation ------------------------------------------------------------------- */
/* replaces the inline GBM block options_model_3.py:473-480 (== Options_model.py:79-88,
 * options_model_2.py:257-264) and the torch loops option_model_3_gpu.py:117-185 */
int omc_gbm_paths_f32(omc_ctx* ctx, float* S, int64_t ld, int64_t n_paths, int n_steps, double S0,
                      double r, double sigma, double T, uint64_t seed, uint64_t stream,
                      uint64_t pair_offset, int antithetic);
/* replaces simulate_heston_paths_antithetic options_model_3.py:211-251
 * (option_model_3_gpu.py:187-248); the variance never reaches memory */
int omc_heston_paths_f32(omc_ctx* ctx, float* S, int64_t ld, int64_t n_paths, int n_steps,
                         double S0, double r, double T, double v0, double kappa, double theta,
                         double xi, double rho, uint64_t seed, uint64_t stream,
                         uint64_t pair_offset, int scheme);
/* omc_heston_paths_f32 with the variance kept: S has the bits of omc_heston_paths_f32 for the same arguments (every
 * scheme), and V [n_steps+1][ld] (device float32, the layout of S: column p and its antithetic partner p + n_paths/2)
 * holds the variance STATE of the same path: row 0 = (float)v0, row t = what the scheme carries into step t + 1 -- scheme
 * 0 floored at 0, scheme 1 unfloored (it may be negative), scheme 2 floored at 1e-8, scheme 3 the sampled v' >= 0.  (S_t, V_t) is the Markov state:
 * omc_heston_paths_from_normals_f32 started at (S[t][j], V[t][j]) with the generator's remaining normals reproduces rows
 * t+1 .. of that pair bit for bit.  The checks of omc_heston_paths_f32, and -7 for a null V -- but with scheme 1 a
 * negative v0 is taken as it is, as omc_heston_paths_from_normals_f32 takes it: a state this generator stores is a state
 * it starts from (the inner paths of omc_price_american_bounds_heston start there; section 21's tests rebuild them so).
 * omc_heston_paths_from_normals_f32 takes a negative v0 with schemes 0, 1 and 2 (0 and 2 floor it before use); it returns
 * -5 for a rho outside [-1, 1] or NaN at every scheme, and for scheme 3 with a v0 that is not >= 0 (NaN included): the
 * moments of QE's next variance need a state >= 0, which is all scheme 3 ever stores.  Nothing is launched then. */
int omc_heston_paths_sv_f32(omc_ctx* ctx, float* S, float* V, int64_t ld, int64_t n_paths, int n_steps,
                            double S0, double r, double T, double v0, double kappa, double theta,
                            double xi, double rho, uint64_t seed, uint64_t stream,
                            uint64_t pair_offset, int scheme);
/* injected-normals parity mode: Zhalf is device float32 [n_steps][ldz], row t-1 drives step t
 * (the exact consumption order of options_model_3.py:475-480 / :223-233) */
int omc_gbm_paths_from_normals_f32(omc_ctx* ctx, float* S, int64_t ld, int64_t n_paths,
                                   int n_steps, double S0, double r, double sigma, double T,
                                   const float* Zhalf, int64_t ldz, int antithetic);
int omc_heston_paths_from_normals_f32(omc_ctx* ctx, float* S, int64_t ld, int64_t n_paths,
                                      int n_steps, double S0, double r, double T, double v0,
                                      double kappa, double theta, double xi, double rho,
                                      const float* Z1half, const float* Z2half, int64_t ldz,
                                      int scheme);
/* RNG taps for known-answer tests: in = n x {ctr[4], key[2]} (host), out = n x 4 (host) */
int omc_philox4x32_10(omc_ctx* ctx, const uint32_t* in, uint32_t* out, int n);
/* the normals the GBM generator consumes: Z device float32 [n_steps][ldz] */
int omc_gbm_normals_f32(omc_ctx* ctx, float* Z, int64_t ldz, int64_t n_pairs, int n_steps,
                        uint64_t seed, uint64_t stream, uint64_t pair_offset);

/* ---- Longstaff-Schwartz backward induction (polynomial regressor) -------------------------- */
/* replaces the backward loops Options_model.py:108-157 / options_model_2.py:278-313
 * (semantics 0), options_model_3.py:482-651 (semantics 2), with the per-step MLP swapped for
 * OLS on [1,u,u^2], u = S/K-1 (the reference accepts lsm_poly_degree and ignores it:
 * Options_model.py:53, options_model_2.py:178-179).
 * betas_out: optional host [n_steps+1][4] = b0,b1,b2,n_itm per step.
 * sx_out / tex_out: optional host [n_paths] final exercise spot / step per path. */
int omc_lsm_poly(omc_ctx* ctx, const float* S, int64_t ld, int64_t n_paths, int n_steps, double K,
                 double r, double T, int is_put, int semantics, omc_result* res,
                 double* betas_out, float* sx_out, int32_t* tex_out);
/* decision replay with given per-step fits (host betas [n_steps+1][4], n<=0 skips the step) */
int omc_lsm_apply_frozen(omc_ctx* ctx, const float* S, int64_t ld, int64_t n_paths, int n_steps,
                         double K, double r, double T, int is_put, const double* betas,
                         omc_result* res, float* sx_out, int32_t* tex_out);

/* the per-step flows (semantics 0 / 1) driven by EXTERNALLY supplied continuation values instead of
 * the fitted polynomial: cont is a device float32 matrix [n_steps+1][ldc] (row t = continuation value of
 * every path at step t, the float32 a torch module returns; entries of paths that are out of the money
 * or, under semantics 0, already exercised are never read).  Replays a recorded run of the reference's
 * own per-step loop -- Options_model.py:108-157 / options_model_2.py:278-313, whose ContNet outputs are
 * the `continuation` of :141-142 -- through the kernel that implements its mask, discounting, strict `>`
 * and (mean, std, zero_prob) statistics. */
int omc_lsm_apply_values(omc_ctx* ctx, const float* S, int64_t ld, int64_t n_paths, int n_steps,
                         double K, double r, double T, int is_put, int semantics, const float* cont,
                         int64_t ldc, omc_result* res, float* sx_out, int32_t* tex_out);

/* The regressor the reference's v1 / v2 pricers run: a FRESH ContNet(1 -> nn_hidden -> nn_hidden -> 1) at
 * every time step (Options_model.py:14-25,112-151; options_model_2.py:283-312, whose constructor arguments
 * nn_hidden / nn_epochs / nn_lr these are): input = the step's regression set (in the money, not yet
 * exercised) standardised by its own mean / population std (std 0: centred only), target = the set's
 * cash-flows valued at the step (not normalised), nn_epochs full-batch Adam(lr = nn_lr) steps on the mean
 * squared error, exercise where payoff > net(input) (strict), sticky mask, cash-flows valued at t = 1.
 * Initialisation is torch's nn.Linear default (uniform +-1/sqrt(fan_in), weights and biases) drawn from
 * Philox keyed by (nn_seed, t): the reference's v1 never seeds torch and its v2 seeds it once per pricing, so
 * individual nets cannot be matched, only the distribution of prices.  nn_hidden 1 .. 128; one GPU (-10 on a
 * context with a communicator or hook).  res->sum_nitm = training rows summed over steps.
 * omc_lsm_contnet works on a device path matrix [n_steps+1][ld]; omc_price_american_contnet generates the
 * paths of `p` first (p->semantics must be OMC_SEM_REFERENCE). */
int omc_lsm_contnet(omc_ctx* ctx, const float* S, int64_t ld, int64_t n_paths, int n_steps, double K, double r,
                    double T, int is_put, int nn_hidden, int nn_epochs, double nn_lr, uint64_t nn_seed,
                    omc_result* res, float* sx_out, int32_t* tex_out);
int omc_price_american_contnet(omc_ctx* ctx, const omc_params* p, int nn_hidden, int nn_epochs, double nn_lr,
                               uint64_t nn_seed, omc_result* res);
/* the initial parameters of step t's net (host float32 [n], n = 8H + H*H + 2H + 1 with H = nn_hidden rounded
 * up to 32 / 64 / 128): layer 0 as [unit][8] = {weight, 0 x 6, bias}, layer 1 as [out][in] then its biases,
 * the output weights, the output bias; entries of units >= nn_hidden are zero.  For tests and for seeding a
 * torch ContNet with the same start. */
int omc_contnet_init_params(omc_ctx* ctx, int nn_hidden, int t, uint64_t nn_seed, float* params_out, int n);

/* multi-GPU: paths shard by antithetic pair, only regression moments and the final sums
 * cross GPUs.  `hook(user, dptr, count)` must all-reduce (sum) `count` DEVICE doubles in place,
 * ordered on the context's stream (RCCL via torch.distributed on the host side).  It is called
 * ONCE with the whole [n_steps+1][8] moment table for the two-pass flow (decision-independent
 * moments), once per time step with 8 doubles for the per-step flows, and finally with the 8
 * result sums {sum, sumsq, n_exercised, n_zero, sum_nitm, ..}.  With a hook installed the
 * returned omc_result therefore carries GLOBAL sums and is normalised by
 * n_paths * world_size (omc_set_option(ctx, "world_size", W); shards are equal). */
typedef int (*omc_allreduce_fn)(void* user, double* dptr, int count);
int omc_set_allreduce_hook(omc_ctx* ctx, omc_allreduce_fn fn, void* user);

/* The same exchange with RCCL called from inside the library (no host callback, no PyTorch):
 * librccl.so is opened on first use.  Rank 0 makes a 128-byte unique id (omc_comm_unique_id) and hands
 * it to the other ranks by any means (options_model_amd/rendezvous.py uses a file on the node); every
 * rank then calls omc_comm_init on its context (collective: ncclCommInitRank on the context's device).
 * From then on the context's pricing calls enqueue ncclAllReduce(sum, double) on its stream for the
 * moment table(s) and the 8 result sums exactly where the hook would have been called, the returned
 * omc_result carries GLOBAL sums, and "world_size" is the communicator's rank count.  The reference has
 * no counterpart (no distributed code: SURVEY.md section 5.8).
 * omc_comm_allreduce_f64: blocking all-reduce of a small HOST vector (op 0 = sum, 1 = max) through the
 * same communicator -- barriers and max-over-ranks timings of a benchmark harness. */
int omc_comm_unique_id(void* uid_out, size_t bytes);
int omc_comm_init(omc_ctx* ctx, int rank, int world, const void* uid, size_t bytes);
int omc_comm_destroy(omc_ctx* ctx);
int omc_comm_info(omc_ctx* ctx, int* rank, int* world); /* world = 0: no communicator */
int omc_comm_allreduce_f64(omc_ctx* ctx, double* host_inout, int count, int op);

/* ---- fused pricing: paths -> LSM -> discounted mean ----------------------------------------- */
/* replaces AdvancedOptionPricer.price_american_enhanced_lsm options_model_3.py:439-651 and
 * price_american_option Options_model.py:44-157 end to end on one GPU.  S_keep: optional
 * caller-owned device matrix [n_steps+1][ld] to receive the paths (NULL: internal workspace) */
int omc_price_american(omc_ctx* ctx, const omc_params* p, omc_result* res, float* S_keep,
                       int64_t ld);
/* Pathwise Greeks of the two-pass (v3) polynomial-LSM estimator with the exercise policy FROZEN:
 * one GPU, p->semantics == OMC_SEM_TWO_PASS, paths stored as omc_price_american stores them (option "fold_antithetic";
 * base.folded says which).  The policy is the fits pass 1 makes at p's parameters, or `betas` (host [n_steps+1][4] =
 * b0, b1, b2, n as omc_lsm_apply_frozen takes them; n <= 0: no exercise at that step; pass 1 is then skipped and
 * base.sum_nitm = 0).  betas_out (NULL or host [n_steps+1][4]) receives the policy used.  One sweep prices three
 * scenarios per path -- S0, S0 (1 + bump), S0 (1 - bump) -- on the stored paths scaled by the factor (every model's spot is
 * proportional to S0) and forms, per path, with s the exercise spot, k the exercise step (N: never), D_k = exp(-r (k-1) dt):
 *   delta D_k phi'(s) s / S0, gamma (delta+ - delta-) / (2 bump S0) from the bumped scenarios' own exercise steps, and for
 *   GBM vega, rho and theta (-dV/dT at fixed n_steps) from the path's Brownian value read back from s.  Heston: vega, rho,
 *   theta and their standard errors are NaN.  Standard errors: sqrt(max(E[x^2] - E[x]^2, 0) / n_paths), antithetic
 *   partners counted as independent paths.  float64 sums in a fixed order: identical calls return identical bits.
 * Errors: -4 semantics != 2 or bump outside (0, 0.5]; -10 context with a communicator or all-reduce hook; -7 null out. */
typedef struct {
    omc_result base;                         /* the pricing, as omc_price_american returns it (ms_pass2 = 0: the sweep
                                                below replaces pass 2)                                               */
    double delta, gamma, vega, rho, theta;   /* raw units: per unit S0 / S0^2 / sigma / r / year                     */
    double se_delta, se_gamma, se_vega, se_rho, se_theta;
    double bump, price_up, price_down;       /* price_up / _down: the frozen-policy prices at S0 (1 +- bump)         */
    int64_t n_exercised_up, n_exercised_down;
    double ms_greeks;                        /* HIP-event time of the Greeks sweep                                   */
} omc_greeks;
int omc_price_american_greeks(omc_ctx* ctx, const omc_params* p, double bump, const double* betas, double* betas_out,
                              omc_greeks* out);
/* Tests of pass 2's exercise tables (option "pass2_tables"): builds the tables of the fits `betas` [n_steps+1][4]
 * (b0, b1, b2, regression-set size; as omc_price_american_greeks returns them) and cK [n_steps+1] (the folded partner's
 * C_t / K) on the device, then compares the table decision with the sweep's float64 decision at every non-negative
 * float32 spot, for the stored path and its partner: mismatches [n_steps+1][2] (host), irregular [n_steps+1] (host: 1 =
 * the step keeps the float64 decisions and is not compared).  irregular_every > 0 forces every k-th step irregular. */
int omc_pass2_tables_check(omc_ctx* ctx, int is_put, double K, int n_steps, const double* betas, const double* cK,
                           int irregular_every, int64_t* mismatches, int* irregular);
/* European discounted payoff from terminal values only (no path matrix): replaces
 * price_european_streaming options_model_3.py:382-437; sums2 host {sum, sumsq} */
int omc_price_european(omc_ctx* ctx, const omc_params* p, omc_result* res);

/* ---- barrier options: knock-in / knock-out, European and American -------------------------- */
/* The reference declares ExoticOptionPricer.price_barrier_option (options_model_2.py:61-67) as a stub; this is it.
 * Paths: p's model, seed, stream and pair_offset, antithetic pairs only (p->antithetic = 1), spots bit-identical to
 * omc_gbm_paths_f32 / omc_heston_paths_f32 wherever the option is live.
 * Monitoring
 *   OMC_MONITOR_DISCRETE    at grid steps t = 1..N: down barriers hit when (double)S_t <= H, up barriers when
 *                           (double)S_t >= H (tested in float32 against the exact float32 threshold).
 *   OMC_MONITOR_CONTINUOUS  GBM only: a partner not yet hit is also hit at step t when u_t < p_t, the Brownian-bridge
 *                           crossing probability p_t = exp2((c x_{t-1}) x_t), c = -2 ln 2 / (sigma^2 dt) in float32,
 *                           x_0 = float32(log2(float32(S0) / H)), x_t = x_{t-1} + (a + b z_t) in float32 -- the spot's own
 *                           log2 increment (a - b z_t for the antithetic partner).  u_t: Philox4x32-10 with key = seed,
 *                           counter = (pair lo, pair hi, 0x80000000 | ((t-1) >> 2), stream), word (t-1) & 3 (x, y, z, w),
 *                           u = (word >> 8) * 2^-24 (box_muller's u2 rule: exact in float32, in [0, 1)); the normals use
 *                           counter word 2 < 2^31, so no uniform shares a counter with a normal.  Both partners of a pair
 *                           share u_t.
 * Conventions: a knock-out is dead AT its hit step (and after), a knock-in is live FROM its hit step on (row 0 of a
 * knock-in is dead).  S0 on or beyond the barrier is an argument error.  No rebate.
 * Encoding (american = 1): the path matrix the two-pass LSM prices holds the real spot where the option is live and the
 * DEAD SPOT elsewhere: the float32 nearest to K on its out-of-the-money side (put: the smallest float32 >= K, call: the
 * largest float32 <= K -- the in-the-money threshold of the sweeps).  Its payoff is <= 0 and it is never in the money, so
 * the unchanged full-storage sweeps exercise a knock-out only before its hit and a knock-in only from its hit on.  The
 * matrix is the library's own or S_keep ([n_steps+1][ld], ld >= n_paths), always full storage (option "fold_antithetic"
 * does not apply: knock state depends on the path).  base = omc_price_american's result on that matrix (folded = 0).
 * american = 0: only the European sums are formed, no matrix is allocated (S_keep, if given, still receives the encoded
 * matrix); base then holds the European option of `kind` (price, sum, sumsq, std, zero_prob; no LSM counts).
 * European sums, on both paths of every pair: payoff of the REAL terminal spot discounted by exp(-r T) (as
 * omc_price_european), knock-out where the partner never hit, knock-in where it hit: euro_in + euro_out is the vanilla
 * European of the same stream, path by path.  Standard errors sqrt(max(E[x^2] - E[x]^2, 0) / n_paths).
 * Errors (nothing is launched): omc_params checks as omc_price_american; -15 unknown kind / monitoring, american not 0/1,
 * or p->antithetic = 0; -11 american with p->semantics != OMC_SEM_TWO_PASS; -12 continuous monitoring under Heston;
 * -13 H not finite and positive; -14 S0 on the knocked side of H; -10 a distributed context (one GPU); -7 null b / out. */
enum { OMC_BARRIER_DOWN_OUT = 0, OMC_BARRIER_UP_OUT = 1, OMC_BARRIER_DOWN_IN = 2, OMC_BARRIER_UP_IN = 3 };
enum { OMC_MONITOR_DISCRETE = 0, OMC_MONITOR_CONTINUOUS = 1 };
typedef struct {
    int32_t kind;        /* OMC_BARRIER_*                                                        */
    int32_t monitoring;  /* OMC_MONITOR_DISCRETE (grid steps 1..N), OMC_MONITOR_CONTINUOUS (GBM) */
    int32_t american;    /* 1: LSM two-pass poly on the encoded matrix; 0: European only          */
    int32_t reserved;
    double H;
} omc_barrier;
typedef struct {
    omc_result base;               /* American: as omc_price_american returns it (folded = 0)             */
    double euro_out, euro_out_se;  /* European knock-out on the same paths                                */
    double euro_in, euro_in_se;    /* European knock-in (euro_in + euro_out = the vanilla, per path)      */
    double hit_prob;               /* fraction of paths that hit the barrier                              */
    double ms_barrier_paths;       /* HIP-event time of the barrier generator (+ its finalize)            */
} omc_barrier_result;
int omc_price_barrier(omc_ctx* ctx, const omc_params* p, const omc_barrier* b, omc_barrier_result* out, float* S_keep,
                      int64_t ld);

/* ---- dividends: a continuous yield and discrete cash / proportional dividends ------------- */
/* omc_price_american on a stock that pays dividends: two-pass flow (p->semantics = OMC_SEM_TWO_PASS), antithetic pairs
 * (p->antithetic = 1), one GPU, GBM and Heston (every scheme), the polynomial regression.
 * Continuous yield q (finite, any sign): the paths drift at rq = p->r - q (one float64 subtraction; the generators' and
 *   the fold table's rate), every discount factor stays at p->r.  A yield-only pricing (n_div = 0) runs
 *   omc_price_american's kernels under its storage rule (option "fold_antithetic"; S_keep forces full storage); with
 *   q = 0 its `base` is omc_price_american's result bit for bit.
 * Discrete dividends d[i] = (t, amount, kind), 0 < t <= T:
 *   OMC_DIV_PROPORTIONAL  amount = delta in [0, 1): the spot becomes s (1 - delta);
 *   OMC_DIV_CASH          amount = c >= 0: the spot becomes max(s - c, 0) -- a dividend is paid only as far as the spot
 *                         covers it, and a spot at 0 stays at 0.
 *   Ex-dividend step k = clamp((int)ceil(t * n_steps / T - 1e-9), 1, n_steps), in float64.  Row k of the path matrix holds
 *   the EX-dividend spot: exercising at step k earns the ex-dividend payoff, the last cum-dividend exercise date is k - 1.
 *   Per-step table, composed on the host in float64: the dividends stable-sorted by k (input order within a step), from
 *   (m, c) = (1, 0): proportional m *= 1 - delta, c *= 1 - delta; cash c += amount; then mul[k] = (float)m, cash[k] =
 *   (float)c.  On a step with an entry, after the model's own step, both partners of a pair become
 *   s = fmaxf(fmaf(s, mul[k], -cash[k]), 0) in float32; the Heston variance is untouched.  Steps without an entry are the
 *   vanilla generator's operations: rows 0 .. first_div_step - 1 carry the bits of omc_gbm_paths_f32 /
 *   omc_heston_paths_f32 at rate rq, and a dividend of amount 0 changes no bit of a non-negative spot.
 *   Any discrete dividend means FULL storage (base.folded = 0), in the library's own matrix or S_keep ([n_steps+1][ld],
 *   ld >= n_paths).  A spot of exactly 0 is an ordinary entry for the sweeps.  A schedule that takes
 *   EVERY path to 0 leaves a singular regression: the result is what the sweeps give for an all-equal column, no more.
 * omc_dividend_schedule: host only (no context, no device work): the argument checks of omc_price_american_div and the
 *   table -- mul, cash, has [n_steps+1] (1 / 0 / 0 where no dividend goes ex; row 0 never has one); any of the three may
 *   be NULL.
 * Errors (nothing is launched): omc_params checks as omc_price_american; -17 q not finite; -18 n_div < 0; -19 d NULL
 * with n_div > 0; -20 a t outside (0, T]; -21 an amount negative or not finite; -22 a proportional amount >= 1; -23 an
 * unknown kind; -24 p->antithetic = 0; -11 p->semantics != OMC_SEM_TWO_PASS; -10 a distributed context (one GPU);
 * -7 null ctx / out; -6 ld < n_paths. */
enum { OMC_DIV_PROPORTIONAL = 0, OMC_DIV_CASH = 1 };
typedef struct {
    double t, amount;    /* ex-dividend time in (0, T]; delta (proportional) or currency units (cash) */
    int32_t kind;        /* OMC_DIV_*                                                                 */
    int32_t reserved;
} omc_dividend;
typedef struct {
    omc_result base;        /* as omc_price_american returns it (folded = 0 with any discrete dividend)            */
    double ms_div_paths;    /* HIP-event time of the path generator of this call                                   */
    int32_t n_div_steps;    /* time steps on which at least one dividend goes ex (0: yield only)                   */
    int32_t first_div_step; /* the first of them (0: none)                                                         */
} omc_div_result;
int omc_dividend_schedule(const omc_params* p, double q, const omc_dividend* d, int n_div, float* mul, float* cash,
                          int32_t* has);
int omc_price_american_div(omc_ctx* ctx, const omc_params* p, double q, const omc_dividend* d, int n_div,
                           omc_div_result* out, float* S_keep, int64_t ld);

/* ---- jump-diffusion: Merton (GBM) and Bates (Heston) paths -------------------------------- */
/* omc_price_american on a stock whose price jumps: compound-Poisson lognormal jumps on top of GBM (Merton) or of any
 * Heston scheme (Bates), with a continuous dividend yield q.  Two-pass flow (p->semantics = OMC_SEM_TWO_PASS),
 * antithetic pairs (p->antithetic = 1), one GPU, the polynomial regression.
 * Parameters: lambda >= 0 jumps per year; a jump multiplies the spot by exp(J), J ~ N(mu_j, sigma_j^2), sigma_j >= 0;
 *   q as in omc_price_american_div.
 * Compensator and drift: kappa = exp(mu_j + sigma_j^2 / 2) - 1; the generator's drift rate is
 *   rj = (p->r - q) - lambda * kappa, formed once in float64 in exactly that order; rj goes wherever the generator takes
 *   a rate, every discount factor stays at p->r.
 * Jump count of a step: exact Poisson by inversion on integers.  With x = lambda * T / n_steps the host builds 16
 *   thresholds in float64: p_0 = exp(-x), p_n = p_{n-1} * x / n, c_n = p_0 + .. + p_n,
 *   thr[n] = min(2^24, floor(c_n * 2^24 + 0.5)) as uint32.  For step t = 1..N of a pair, w = the top 24 bits (word >> 8)
 *   of word (t-1) & 3 of the Philox4x32-10 block at counter (pair lo, pair hi, 0x40000000 | ((t-1) >> 2), stream), key =
 *   the seed as everywhere; the count is n = #{k : w >= thr[k]}, 0 .. 16.  x > 1 is refused (at x = 1 the mass beyond 16
 *   jumps is below 1e-14).  The normals use counter word 2 below 2^30 and the barrier's uniforms 0x80000000 | blk, so
 *   the families never share a counter.
 * Jump size, only where n > 0: z_J = the first value of box_muller(o.x, o.y) of the Philox block o at counter
 *   (pair lo, pair hi, 0xC0000000 | t, stream); the log2 jump in float32 is
 *   jl = fmaf(sqrtf((float)n) * sj2, z_J, (float)n * mj2), mj2 = (float)(mu_j log2 e), sj2 = (float)(sigma_j log2 e).
 * Both partners of a pair share n and z_J: only the diffusion is antithetic.
 * Step rule: GBM s *= exp2(fma(b, z, a) + jl), partner s' *= exp2(fma(-b, z, a) + jl); Heston, after the scheme's own
 *   step, s *= exp2(jl) and s' *= exp2(jl), the variance untouched.  A step with n = 0 executes the vanilla generator's
 *   operations and nothing else: every column carries the bits of omc_gbm_paths_f32 / omc_heston_paths_f32 at rate rj up
 *   to its own first jump, and with mu_j = sigma_j = 0 no bit differs from the vanilla matrix at rate p->r - q for any
 *   lambda.
 * lambda = 0 delegates to the yield-only route of omc_price_american_div (its storage rule, omc_price_american's bits at
 *   q = 0); any lambda > 0 means FULL storage (base.folded = 0), in the library's own matrix or S_keep
 *   ([n_steps+1][ld], ld >= n_paths): with jumps the partner's spot is no function of the stored one.
 * omc_jump_table: host only (no context, no device work): the argument checks of omc_price_american_jump and the table;
 *   any of thr, kappa, drift_rate may be NULL.
 * Errors (nothing is launched): omc_params checks as omc_price_american; -25 j NULL; -17 q not finite; -26 lambda
 * negative or not finite; -27 mu_j not finite, or sigma_j negative or not finite; -28 lambda * T / n_steps > 1;
 * -24 p->antithetic = 0; -11 p->semantics != OMC_SEM_TWO_PASS; -10 a distributed context (one GPU); -7 null ctx / out;
 * -6 ld < n_paths. */
typedef struct {
    double lambda, mu_j, sigma_j; /* jumps per year; mean and standard deviation of a jump's log size */
} omc_jump;
typedef struct {
    omc_result base;       /* as omc_price_american returns it (folded = 0 with lambda > 0)                        */
    double ms_jump_paths;  /* HIP-event time of the path generator of this call                                    */
    double kappa;          /* exp(mu_j + sigma_j^2 / 2) - 1                                                        */
    double drift_rate;     /* rj = (r - q) - lambda kappa                                                          */
    int32_t n_thresholds;  /* entries of the table below 2^24: the largest count a step can carry (0: lambda = 0)  */
    int32_t reserved;
} omc_jump_result;
int omc_jump_table(const omc_params* p, const omc_jump* j, double q, uint32_t thr[16], double* kappa,
                   double* drift_rate);
int omc_price_american_jump(omc_ctx* ctx, const omc_params* p, const omc_jump* j, double q, omc_jump_result* out,
                            float* S_keep, int64_t ld);

/* ---- multi-asset options: basket, best-of and worst-of ------------------------------------ */
/* omc_price_american on an INDEX X_t of d correlated GBM assets, 1 <= d <= 8: the payoff is max(K - X, 0) (p->is_put) or
 * max(X - K, 0), and the two-pass flow regresses on [1, u, u^2] of the index -- the exercise policy is a function of the
 * index alone.  Two-pass flow (p->semantics = OMC_SEM_TWO_PASS), antithetic pairs (p->antithetic = 1), one GPU, GBM
 * (p->model = OMC_MODEL_GBM), FULL storage (base.folded = 0).  K, is_put, r, T, the sizes, seed, stream and pair_offset
 * come from omc_params; p->S0 and p->sigma are NOT read (the omc_params checks run on a copy that carries X_0 and sigma[0]
 * in their place).
 * Per asset i: S0[i] > 0, sigma[i] > 0, a continuous yield q[i] (finite, any sign), a weight w[i] > 0 (finite, not
 *   normalised); rho[i * d + j] is the correlation matrix, row-major in the first d * d entries; kind is OMC_BASKET_*.
 * Host constants, float64 then rounded once: dt = T / n_steps; rq_i = p->r - q[i];
 *   a_i = (float)((rq_i - sigma_i^2 / 2) dt log2 e), b_i = (float)(sigma_i sqrt(dt) log2 e) -- omc_gbm_paths_f32's at rate
 *   rq_i; wf_i = (float)w[i], s0f_i = (float)S0[i]; L = the lower Cholesky factor of rho, row by row (Cholesky-Banachiewicz:
 *   for j <= i, t = rho[i][j] - sum_{k<j} L[i][k] L[j][k], k ascending; L[i][i] = sqrt(t), L[i][j] = t / L[j][j]), from the
 *   lower triangle of rho, Lf = (float)L.  rho is refused when an entry is not finite, a diagonal entry is off 1 by more
 *   than 1e-12, |rho[i][j] - rho[j][i]| > 1e-12, or a pivot t is <= 1e-12.
 * Normals: asset k of pair p at Philox block blk takes the four normals of the vanilla GBM generator at the pair index
 *   pair_offset + p + ((uint64_t)k << 40), counter word 2 = blk: the asset tag sits in the PAIR index, so the tagged
 *   families of the barrier and jump generators are untouched, asset k's independent normals are omc_gbm_normals_f32's at
 *   pair_offset + (k << 40), and a call with pair_offset + n_paths / 2 > 2^40 is refused.
 * Correlation, float32, fixed order: y_i = Lf[i][0] z_0, then y_i = fmaf(Lf[i][k], z_k, y_i), k = 1 .. i (Lf[0][0] is
 *   1.0f exactly, so y_0 = z_0).
 * Step: e_i = fmaf(b_i, y_i, a_i), s_i *= exp2(e_i); the partner flips EVERY asset's normal: e'_i = fmaf(-b_i, y_i, a_i),
 *   s'_i *= exp2(e'_i) -- omc_gbm_paths_f32's step per asset.
 * Index, float32, from the registers the asset rows are stored from:
 *   OMC_BASKET_ARITHMETIC  X = wf_0 s_0, then X = fmaf(wf_k, s_k, X), k ascending;
 *   OMC_BASKET_BEST_OF     X = wf_0 s_0, then X = fmaxf(X, wf_k s_k);   OMC_BASKET_WORST_OF the same with fminf;
 *   OMC_BASKET_GEOMETRIC   a state of its own: g_0 = (float)prod_i S0[i]^w[i] (float64 product, i ascending), and per step
 *                          g *= exp2(E), E = wf_0 e_0, then E = fmaf(wf_k, e_k, E) (the partner from its own e'_k).
 *   Row 0 holds the index of the initial spots by the same rule (geometric: g_0).
 *   OMC_BASKET_ASIAN_ARITHMETIC / _GEOMETRIC: the running average of the BASKET VALUE over the grid
 *     dates 1 .. t (S_0 is not in it) -- a fixed-strike average-price option with early exercise; with d = 1 and w = 1 the
 *     basket value is the spot, the plain Asian option.  B_t = the value of step t by OMC_BASKET_ARITHMETIC's rule exactly
 *     (wf_0 s_0, then fmaf(wf_k, s_k, B), k ascending); inv_t = 1.0f / (float)t, an IEEE correctly rounded float32 division.
 *       _ARITHMETIC  c_0 = 0, c_t = c_{t-1} + B_t (ONE float32 add, not contracted with the product of B), X_t = c_t * inv_t;
 *       _GEOMETRIC   l_0 = 0, l_t = l_{t-1} + log2(B_t) (the hardware log2, v_log_f32), X_t = exp2(l_t * inv_t) (v_exp_f32);
 *     X_0 = B_0 for both.  The partner of a pair keeps its own c or l.  The arithmetic rule can be restated bit for bit in
 *     float32 from the asset matrices; the geometric one is compared by tolerance (4.5e-6 relative at 252 dates).
 * Storage: the index goes to the context's full-storage matrix or to S_keep ([n_steps+1][ld], ld >= n_paths); with
 *   assets_keep the per-asset matrices go to that buffer, [d][n_steps+1][ld] (the same ld; without S_keep, ld as passed).
 *   Columns p and p + n_paths / 2 are the partners, as everywhere else.
 * What follows: with d = 1, w = 1 and any kind the index matrix is omc_gbm_paths_f32's at rate r - q[0], bit for bit;
 *   with rho = I asset k's matrix is omc_gbm_paths_f32(S0[k], r - q[k], sigma[k], pair_offset + (k << 40)), bit for bit,
 *   and asset 0's is that for any rho; the geometric index is a GBM from G_0 = prod S0[i]^w[i] with
 *   sigma_G^2 = sum_ij w_i w_j sigma_i sigma_j rho_ij and yield q_G = r - sum_i w_i (r - q_i - sigma_i^2 / 2) - sigma_G^2 / 2.
 * The default flow is the reference's two-pass rule, which sits above the Andersen-Broadie upper bound for a vanilla put
 *   (DESIGN.md section 12): these prices are not comparable with literature tables of textbook LSM.
 * omc_basket_table: host only (no context, no device work): the argument checks of omc_price_american_basket and the
 *   constants -- L_packed [d (d+1) / 2] (row i at i (i+1) / 2, float64), a, b [d], x0 (the index of the initial spots in
 *   float64: sum w_i S0_i, max / min of w_i S0_i, or G_0; the Asian kinds: sum w_i S0_i), geo [3] = G_0, sigma_G, q_G (for
 *   every kind those of OMC_BASKET_GEOMETRIC); any output may be NULL.
 * Errors (nothing is launched): -7 null ctx / params / out; -12 p->model not GBM; -29 basket NULL or n_assets outside
 * 1 .. 8; -30 a bad per-asset field; -32 unknown kind; -31 rho refused; then the omc_params checks as omc_price_american
 * (on the copy); -24 p->antithetic = 0; -11 p->semantics != OMC_SEM_TWO_PASS; -33 pair_offset + n_paths / 2 > 2^40;
 * -10 a distributed context (one GPU); -6 ld < n_paths (S_keep or assets_keep given). */
enum { OMC_BASKET_ARITHMETIC = 0, OMC_BASKET_GEOMETRIC = 1, OMC_BASKET_BEST_OF = 2, OMC_BASKET_WORST_OF = 3,
       OMC_BASKET_ASIAN_ARITHMETIC = 5, OMC_BASKET_ASIAN_GEOMETRIC = 6 }; /* 4 is not a kind: it stays refused (-32) */
#define OMC_BASKET_MAX_ASSETS 8
typedef struct {
    int32_t n_assets, kind;                 /* d in 1 .. 8; OMC_BASKET_*                                       */
    double S0[8], sigma[8], q[8], w[8];     /* per asset: spot, volatility, continuous yield, weight           */
    double rho[64];                         /* correlation matrix, row-major [d][d] in the first d * d entries */
} omc_basket;
typedef struct {
    omc_result base;        /* as omc_price_american returns it on the index matrix (folded = 0)                   */
    double ms_basket_paths; /* HIP-event time of the path generator of this call                                   */
    double index0;          /* the index of the initial spots, float64 (x0 of omc_basket_table)                    */
    int32_t n_assets, kind;
} omc_basket_result;
int omc_basket_table(const omc_params* p, const omc_basket* b, double* L_packed, float* a, float* b_out, double* x0,
                     double* geo);
int omc_price_american_basket(omc_ctx* ctx, const omc_params* p, const omc_basket* b, omc_basket_result* out,
                              float* S_keep, float* assets_keep, int64_t ld);

/* ---- frozen-policy pathwise Greeks of the multi-asset options ------------------------------ */
/* omc_price_american_greeks for omc_price_american_basket: per-asset delta, diagonal gamma and vega, and rho and theta of
 * the option, with the exercise policy FROZEN.  Scope as omc_price_american_basket (its checks run unchanged): GBM assets,
 * two-pass flow, antithetic pairs, one GPU, full storage, d = 1 .. 8, kinds 0 .. 3.  The Asian kinds are refused: the
 * sweep regenerates the asset spots and would need the running state beside them.
 * Policy: the [1, u, u^2] fits pass 1 makes on the index matrix at p's and b's parameters, or `betas` (host
 *   [n_steps+1][4] = b0, b1, b2, n; n <= 0: no exercise at that step; an all-zero table gives European Greeks).  With
 *   `betas` the generator and pass 1 are skipped, no matrix is written and base.base.sum_nitm = 0.  betas_out (NULL or host
 *   [n_steps+1][4]) receives the policy used.
 * Paths: ONE sweep regenerates the spots omc_price_american_basket's generator stores, bit for bit (the section above),
 *   and walks every path forward.  Below, of a path at step t: s_i = (double) of the float32 spot of asset i, X = (double)
 *   of the float32 index, p_i = (double)(wf_i * s_i), the float32 product the best-of / worst-of index compares.
 * Exercise step k of a path: pass 2's -- the latest t in 1 .. N-1 at which the payoff phi(X) = K - X (put) / X - K (call)
 *   is positive and above the fit at u = X / K - 1, else N.  D_k = exp(-r (k-1) dt), cf = D_k max(phi(X), 0) (the pricing's
 *   cash-flow), phi' = -1{phi > 0} (put) / +1{phi > 0} (call), all at step k.
 * Partials x_i = dX/ds_i s_i, float64, at step k:
 *   OMC_BASKET_ARITHMETIC  x_i = (double)wf_i s_i;      OMC_BASKET_GEOMETRIC  x_i = (double)wf_i X;
 *   OMC_BASKET_BEST_OF / _WORST_OF  x_i = p_i if i is the lowest asset number whose float32 product equals the float32
 *   index, else 0.
 * Per asset i:  delta_i = D_k phi'(X) x_i / S0_i;
 *   vega_i = D_k phi'(X) x_i (ln(s_i / S0_i) - (r - q_i + sigma_i^2 / 2) k dt) / sigma_i  (the correlated Brownian value of
 *   asset i is a function of its own spot and does not depend on sigma_j).
 * Of the option:  rho = -(k-1) dt cf + D_k phi'(X) k dt sum_i x_i;
 *   theta = -[ -r (k-1) dt / T cf + D_k phi'(X) sum_i x_i (ln(s_i / S0_i) + (r - q_i - sigma_i^2 / 2) k dt) / (2 T) ]
 *   (-dV/dT at fixed n_steps).  With d = 1, w = 1, q = 0 these are omc_price_american_greeks' expressions.
 * Diagonal gamma (want_gamma != 0), h = bump: scenario i+- scales asset i ALONE by lambda = 1 +- h, forms its own float64
 *   index at every step, decides with the same fits and keeps its own exercise step k_i+-.  The scenario index:
 *   arithmetic  X + (+-h (double)wf_i) s_i (one fma);   geometric  X c_i+-, c_i+- = pow(1 +- h, (double)wf_i) (host);
 *   best-of / worst-of  max / min of lambda p_i and m_i, m_i = (double) of the float32 max / min of the OTHER assets'
 *   products (none: -inf / +inf).
 *   delta_i+- = D_k+- phi'(X^i+-) x_i^+- / S0_i with x_i^+- UNSCALED at the scenario's own step: (double)wf_i s_i,
 *   (double)wf_i X, or p_i where the scaled asset carries the scenario index (lambda p_i >= m_i, worst-of <=; a tie goes
 *   to the scaled asset), else 0.  gamma_i = (delta_i+ - delta_i-) / (2 h S0_i); price_up[i] / price_down[i] = the means
 *   of D_k+- max(phi(X^i+-), 0); n_exercised_up / _down[i] count k_i+- < N.  Without want_gamma: gamma, se_gamma, price_up
 *   and price_down are NaN, the scenario counts 0, and every other field has the bits of the call with want_gamma.
 * Standard errors: sqrt(max(E[x^2] - E[x]^2, 0) / n_paths), antithetic partners counted as independent paths.  float64
 *   sums, per-workgroup partials, a finalize in workgroup order: identical calls return identical bits.
 * base: omc_price_american_basket's result (counts identical, price up to the order of its float64 sum) with
 *   ms_pass2 = 0: the sweep replaces pass 2.  Entries of the per-asset arrays at or above d are 0.
 * Out of scope: cross-gammas, correlation and yield sensitivities, Heston or jump assets, the runner-up policy.
 * Errors (nothing is launched): omc_price_american_basket's own, in its order (-7 null ctx / out / params, -12, -29 .. -32,
 * the omc_params checks, -24, -11, -33); then -32 kind OMC_BASKET_ASIAN_ARITHMETIC / _GEOMETRIC; -4 bump outside (0, 0.5];
 * -10 a distributed context (one GPU). */
typedef struct {
    omc_basket_result base;
    double delta[8], gamma[8], vega[8];        /* raw units: per unit S0_i / S0_i^2 / sigma_i                         */
    double se_delta[8], se_gamma[8], se_vega[8];
    double rho, theta, se_rho, se_theta;       /* per unit r / per year                                               */
    double bump, price_up[8], price_down[8];   /* the frozen-policy prices at S0_i (1 +- bump)                        */
    int64_t n_exercised_up[8], n_exercised_down[8];
    double ms_greeks;                          /* HIP-event time of the Greeks sweep                                  */
    int32_t gamma_on, reserved;
} omc_basket_greeks;
int omc_price_american_basket_greeks(omc_ctx* ctx, const omc_params* p, const omc_basket* b, double bump, int want_gamma,
                                     const double* betas /* NULL or host [n_steps+1][4] */,
                                     double* betas_out /* NULL or host [n_steps+1][4] */, omc_basket_greeks* out);

/* ---- Andersen-Broadie price bounds for American options ----------------------------------- */
/* A lower and an upper bound on the value of the Bermudan put / call on the pricing grid, both from ONE frozen exercise
 * policy: the lower bound applies the policy as a stopping rule on fresh paths, the upper bound is the Andersen-Broadie
 * (2004) dual estimator whose martingale comes from nested inner simulations.  GBM only, one GPU.
 * The game: exercise dates t = 1..N on the grid dt = T / N; every value is discounted to t = 0,
 *     Z_t = exp(-r t dt) max(phi(S_t), 0)
 * -- the textbook convention, NOT the reference flows' valuation at t = dt (omc_result.price of semantics 0 / 2).
 * The policy: a table betas [N+1][4] = (b0, b1, b2, n) as omc_lsm_poly returns it.  At t in 1..N-1 a path at spot s
 * exercises iff n_t > 0.5 (a regression-set size), imm = phi(s) > 0 and imm > fma(u, fma(u, b2, b1), b0) with
 * u = fma((double)s, 1/K, -1) -- omc_lsm_apply_frozen's float64 rule; at t = N it takes its payoff.  tau_t = the FIRST
 * date >= t at which the rule fires (a stopping time).  The kernels decide from pass 2's float32 exercise tables
 * (omc_crit.h, stored-path kind) on the steps the builder certifies and with the float64 rule on the others: the same
 * decisions.
 * policy (omc_bounds_config.policy): OMC_SEM_REFERENCE / OMC_SEM_TEXTBOOK / OMC_SEM_TWO_PASS = the fits omc_lsm_poly
 * makes with that semantics on p->n_paths paths generated at (p->seed, p->stream, p->pair_offset, p->antithetic) --
 * textbook is the best policy of the three; OMC_POLICY_GIVEN = the caller's table `betas`.  p->semantics is not used.
 * Lower bound: n_lower paths of omc_gbm_paths_f32(n_lower, N, S0, r, sigma, T, seed, stream_lower, pair_offset 0,
 * antithetic): the mean of Z at tau_1; its standard error from PAIR means (the two partners of a pair averaged first).
 * Upper bound: n_outer outer paths of omc_gbm_paths_f32(.., stream_outer, ..) likewise.  For outer path i and t = 0..N-1,
 *     Q^_t[i] = mean of Z at tau_{t+1} over n_inner inner paths started at S_t[i]
 * Inner pair j of (i, t) is generator pair g = (i (N+1) + t) (n_inner/2) + j of Philox stream stream_inner; inner step
 * k = 1..N-t consumes that pair's generator row k-1 (omc_gbm_normals_f32), the partner -z, and the spot recurrence is
 * the generator's own (s = s * exp2(fma(+-b, z, a)) from the float32 S_t[i]): the inner spots are bit for bit
 * omc_gbm_paths_from_normals_f32(z, S0 = S_t[i], r, sigma, T) with z = omc_gbm_normals_f32(n_inner/2, N, seed,
 * stream_inner, pair_offset = (i (N+1) + t) n_inner/2) (rows after N-t unused).  Then per outer path
 *     L^_t = Z_t if the policy exercises at t or t = N, else Q^_t  (t >= 1);   M^_0 = 0, M^_t = M^_{t-1} + L^_t - Q^_{t-1}
 *     sample_i = max_{t=1..N} (Z_t - M^_t)
 * upper = mean of the samples, se_upper from pair means (i and i + n_outer/2).  ci = [lower - 1.96 se_lower,
 * upper + 1.96 se_upper].  The inner noise has conditional mean 0, so the upper estimate is biased upward only.
 * Outputs: betas_out (NULL or host [N+1][4]) the policy used; q_out (NULL or host [n_outer][N]) the Q^_t; samples_out
 * (NULL or host [n_outer]) the samples.  n_exercised_lower: lower paths stopped before N.  inner_path_steps: the steps
 * the inner paths took, sum over all inner paths of (tau - t).  ms_*: HIP-event times of the policy fit, the lower
 * sweep, the upper bound (outer paths, exercise tables, inner simulations, outer walk) and the whole call.  float64
 * sums in a fixed order: identical calls return identical bits.  The inner simulations run as launches over blocks of
 * outer paths, each bounded in work.
 * Errors (nothing is launched): omc_params checks as omc_price_american; -12 a model other than GBM; -10 a context with
 * a communicator or all-reduce hook; -4 policy not one of the four; -3 n_lower, n_outer or n_inner odd or < 2;
 * -16 n_outer (N+1) n_inner above 2^32 or n_outer n_inner N (N+1) / 2 (the inner steps of a policy that never
 * exercises) above 2^39; -7 null cfg / out, or betas NULL with OMC_POLICY_GIVEN.
 *
 * ---- ... with an exercise schedule ----
 * Option "bounds_exercise_every" = k (omc_set_option; a context option because omc_bounds_config has no free field and the
 * entry points are frozen: no new symbol, the same struct layout, OMC_ABI_VERSION unchanged).  k = 0 (default) or 1:
 * everything above, bit for bit.  k >= 2 changes the GAME, not a route: the option whose value is bounded may be exercised at
 *     tau_j = N - (J - j) k,  j = 1 .. J,  J = (N - 1) / k + 1      (the dates t in 1..N with (N - t) % k == 0; tau_0 = 0)
 * -- every k-th date counted back from expiry, omc_chain_entry::exercise_every's anchoring, and the expiry itself; k >= N
 * leaves the expiry alone (J = 1, the European option).  Z_t = D[t] max(phi(S_t), 0) at the scheduled t, the same discount.
 * Paths: the fine grid's in every sweep.  The lower, outer and inner paths keep their Philox coordinates exactly; inner pair
 *   j' of item (i, t) is still generator pair (i (N+1) + t) (n_inner/2) + j' of stream_inner, its blocks counted from the
 *   item's start, so an inner path of a scheduled item is bit for bit the inner path the all-dates call simulates at (i, t).
 * Policy: the table stays betas [N+1][4].  Rows off the schedule count as n = 0 whatever they hold and come back as zero
 *   rows in betas_out (row 0 and row N included: no rule is read there).  OMC_POLICY_GIVEN: the caller's scheduled rows.
 *   Fitted: rows 0, tau_1 .. tau_J of the p->n_paths fitting paths are gathered into a matrix [J+1][ld] and omc_lsm_poly's
 *   fit of that semantics runs on it with J steps and horizon T_v = T when J k == N, else T (double)(J k) / (double)N (a
 *   short first gap counts as a whole one); fit row j becomes row tau_j.  The scheduled rows of betas_out carry the bits
 *   omc_lsm_poly returns for that matrix, (J, T_v) and the same K, r, is_put.
 * Lower bound: the sweep above on the tables of that policy; a zero row never stops a path.
 * Upper bound: inner simulations at the dates tau_0 .. tau_{J-1} only,
 *     Q^_j[i] = mean of Z at the first scheduled date > tau_j where the rule fires (else N), over n_inner inner paths started
 *               at the outer state at tau_j
 *     M_0 = 0,  M_j = M_{j-1} + L_j - Q^_{j-1},  L_j = Z_{tau_j} if the policy exercises at tau_j or j = J, else Q^_j
 *     sample_i = max_{j=1..J} (Z_{tau_j} - M_j)
 * q_out keeps its shape [n_outer][N]: column tau_j holds Q^_j, every other column 0.0.  inner_path_steps counts steps of
 *   the fine grid, as above; at most n_outer n_inner sum_{j<J} (N - tau_j).  The -16 limits stay the all-dates formulas
 *   above, which is conservative: a scheduled call does less work than they allow for.  Option
 *   "pass2_tables_irregular_every" acts as above.  Identical calls return identical bits.
 * With the policy P of an all-dates call masked to the schedule (rows off it zeroed) and given to an all-dates call, that
 *   call's lower, se_lower, n_exercised_lower and its Q^ at the columns tau_j equal the scheduled call's bit for bit.
 * Taken by omc_price_american_bounds and by omc_price_american_bounds_heston with cfg->regressors = OMC_HESTON_REG_SPOT.
 * Error -38 (k >= 2 only; after the call's own argument checks, nothing is launched, the outputs are untouched): the
 *   spot + variance policy of omc_price_american_bounds_heston, omc_price_american_basket_bounds (the Asian kinds included)
 *   and omc_price_american_basket_bounds_runnerup take no schedule.  Entry points that compute no bounds ignore the option.
 *
 * ---- ... with the Black-Scholes control variate ----
 * Option "bounds_control_variate" = v (omc_set_option; a context option for the reasons above: no new symbol, the same struct
 * layout, OMC_ABI_VERSION unchanged).  v = 0 (default): everything above, bit for bit, and the same launches.  v = 1: the
 * controlled estimators below.  Any other value is refused with -4 and the stored value stays.
 * Inputs: dt = T / N in double, D[t] the discount table above, x = (double)s for a float32 spot s.  E(x, d) is the
 *   Black-Scholes value (no dividend yield) of the European put / call at spot x, strike K, rate r, volatility sigma and time
 *   to expiry (N - d) dt, in float64 with Phi(y) = erfc(-y / sqrt 2) / 2:
 *     d1 = (log(x / K) + (r + sigma^2 / 2) tau) / (sigma sqrt tau),  d2 = d1 - sigma sqrt tau,  tau = (N - d) dt
 *     put: K exp(-r tau) Phi(-d2) - x Phi(-d1)        call: x Phi(d1) - K exp(-r tau) Phi(d2)
 *   D_t E(S_t, t) is a martingale on the grid, so D_tau E(S_tau, tau) - D_t E(S_t, t) has conditional mean zero for every
 *   stopping time tau of the policy (the inner control variate of Andersen-Broadie 2004, section 5).
 * Paths, stopping rule, Philox coordinates, policy, exercise tables, walk and Z are unchanged; only what is averaged changes.
 *   Controlled term: a partner stopped at index x and date d contributes c = Z - D[d] E(x, d) when d < N, and exactly 0.0,
 *     with nothing evaluated, when d = N.
 *   Inner items: Q^_t[i] = D[t] E(S_t[i], t) + (1 / n_inner) sum of c over the item's inner paths.  q_out holds these values;
 *     the walk is the one above, scheduled or not, reading them.
 *   Lower bound: the device sums the centred pair means (c_a + c_b) / 2 and their squares; lower = E0 + their mean with
 *     E0 = D[0] E((double)(float)S0, 0) formed on the host in double, and se_lower comes from the centred pair means alone.
 *     n_exercised_lower is unchanged.
 *   With the same arguments betas_out, n_exercised_lower and inner_path_steps equal the plain call's exactly: the same
 *     paths, the same stops.
 *   Validity: the inner estimate stays conditionally unbiased, so `upper` is still biased upward only.  (The control's mean
 *     is zero up to the float32 rounding of the generator's step constants, of the order of 1e-7 relative: five orders below
 *     any standard error the call can reach.)
 *   float64 sums in a fixed order: identical calls return identical bits.  The inner sweep gives an item a group of G = 8,
 *     16, 32 or 64 lanes (the smallest G >= n_inner / 2, at most 64); an inner pair's Philox coordinates do not depend on G.
 * Taken by omc_price_american_bounds: all four policies, the all-dates game and a schedule ("bounds_exercise_every" >= 2).
 * Error -39 (v = 1 only; after the call's own argument checks, behind -16 and -38; nothing is launched, the outputs are
 *   untouched): omc_price_american_bounds_heston (both regressor sets), omc_price_american_basket_bounds (the Asian kinds
 *   included) and omc_price_american_basket_bounds_runnerup have no control variate.  With the option back at 0 they return
 *   their old bits.  Entry points that compute no bounds ignore the option.
 * Option "bounds_cv_form" (for the library's tests and timing tool only: unsupported, and it may vanish without an ABI bump;
 *   0 = default, the lane groups above): 1 = one item per wave, G = 64 whatever n_inner.  The same Q^ up to the order of the
 *   float64 sums.  Another value is refused with -4.
 *
 * ---- ... with sub-optimality checking (Broadie-Cao 2008) ----
 * Option "bounds_suboptimality" = m (omc_set_option; a context option for the reasons above: no new symbol, the same struct
 * layout, OMC_ABI_VERSION unchanged).  m = 0 (default, "off"): everything above, bit for bit, and the same launches.  m = 1
 * ("payoff") and m = 2 ("European"): the rule below.  Any other value is refused with -4 and the stored value stays.
 * Symbols: s = So[t][i], the float32 index of outer path i at date t; x = (double)s; phi(x) = K - x for a put and x - K for a
 *   call; stop(s, t) the decision of the frozen policy (the exercise tables, the float64 rule on irregular dates).
 * Which items are kept: item (i, t), 0 <= t < N, is KEPT iff one of
 *     t == 0;    stop(s, t);    m == 1 and phi(x) > 0;
 *     m == 2 and phi(x) > E(x, t), E the Black-Scholes value of the control variate's section, formed in float64 from its
 *                table of per-date constants (built for this purpose alone when the control variate is off) and evaluated as
 *                not (phi(x) <= E(x, t)), so that a NaN keeps the item.
 *   The expiry t = N is always a date of the walk.  The stop rule requires a positive payoff, so in mode 1 a skipped item
 *   is never one at which the policy stops; in mode 2 an item at which the policy stops is kept whatever E says.  There is no
 *   "local policy fixing": the policy, the exercise tables and the lower bound stay exactly as they are.
 * Inner simulations run for kept items only, with the item's Philox coordinates (gbase = (i (N+1) + t) n_inner / 2 on
 *   stream_inner), lane assignment and fixed-order sum: Q^_t[i] of a kept item has the BITS of the unchecked call's value,
 *   for the plain estimator and for the controlled one (the same lane group G).  q_out keeps its shape [n_outer][N]; a
 *   skipped item's entry is 0.0.  inner_path_steps counts the kept items' steps only.
 * Walk, per outer path: M = 0, lq = Q^_0; for t = 1 .. N, only at kept dates and at t = N:
 *     L = stop ? Z_t : Q^_t  (Q^_N = 0);    M = M + L - lq;    candidate Z_t - M;    lq = Q^_t.
 *   The sample is the maximum of the candidates.  Between two kept dates the policy continues, so the dense walk's
 *   increments sum to L_k - Q^_l exactly: the kept-date M is the dense M up to rounding, and when every item is kept the
 *   checked walk returns the dense walk's bits.
 * Still an upper bound: at a skipped date Z_t <= D_t E_t <= the continuation value (mode 1: Z_t = 0), so the game without
 *   those exercise rights has the same value, the dual bound holds for that game with any martingale, and the inner noise
 *   still biases upward only.  Each sample is at most the unchecked one up to the walk's rounding.
 * Taken by the all-dates game of omc_price_american_bounds (plain and with "bounds_control_variate" = 1, all four policies;
 *   m = 1 and m = 2), omc_price_american_basket_bounds (the Asian kinds included; m = 1) and omc_price_american_bounds_heston
 *   with regressors OMC_HESTON_REG_SPOT (m = 1).
 * Error -40 (after the call's own argument checks, behind -16, -38 and -39; nothing is launched, the outputs are untouched):
 *   m >= 1 while "bounds_exercise_every" >= 2; m >= 1 on a flow with a policy of its own (omc_price_american_bounds_heston
 *   with the spot + variance policy, omc_price_american_basket_bounds_runnerup for the runner-up and for the Asian index +
 *   spot); m = 2 on any entry point other than omc_price_american_bounds.  With the option back at 0 they return their old
 *   bits.  Entry points that compute no bounds ignore the option. */
enum { OMC_POLICY_GIVEN = 3 };
typedef struct {
    int32_t policy;    /* OMC_SEM_REFERENCE, OMC_SEM_TEXTBOOK, OMC_SEM_TWO_PASS: fitted here; OMC_POLICY_GIVEN: `betas` */
    int32_t regressors; /* omc_price_american_bounds_heston: OMC_HESTON_REG_SPOT (0) or OMC_HESTON_REG_SPOT_VARIANCE; the
                          other three bounds entry points do not read it (it was a reserved field: callers zero it) */
    int64_t n_lower, n_outer, n_inner;
    uint64_t stream_lower, stream_outer, stream_inner;
} omc_bounds_config;
typedef struct {
    double lower, se_lower, upper, se_upper, ci_lo, ci_hi; /* ci: lower - 1.96 se_lower, upper + 1.96 se_upper */
    int64_t n_lower, n_outer, n_inner, n_exercised_lower, inner_path_steps;
    double ms_fit, ms_lower, ms_upper, ms_total;
} omc_bounds;
int omc_price_american_bounds(omc_ctx* ctx, const omc_params* p, const omc_bounds_config* cfg,
                              const double* betas /* policy == OMC_POLICY_GIVEN: host [N+1][4] */, double* betas_out,
                              double* q_out /* NULL or host [n_outer][N]: Q^_t, for tests */,
                              double* samples_out /* NULL or host [n_outer] */, omc_bounds* out);

/* ---- Andersen-Broadie price bounds for multi-asset American options ------------------------ */
/* omc_price_american_bounds on the INDEX X_t of d correlated GBM assets, 1 <= d <= 8, arithmetic basket, best-of or
 * worst-of: a lower and an upper bound on the Bermudan value of the game Z_t = exp(-r t dt) max(phi(X_t), 0), t = 1..N,
 * both from one frozen policy that is a function of the index alone.  What the bounds bracket is the TRUE value of the
 * multi-asset game (any policy); how far the lower bound sits below it is what the index-alone policy costs.
 * Arguments: p and b as omc_price_american_basket takes them (its checks run unchanged: GBM, antithetic = 1,
 *   p->semantics = OMC_SEM_TWO_PASS, pair_offset + n_paths / 2 <= 2^40; p->S0, p->sigma not read); cfg, betas, betas_out,
 *   q_out, samples_out as omc_price_american_bounds takes them.
 * Policy: the rule of omc_lsm_apply_frozen on u = X / K - 1 with a table betas [N+1][4].  cfg->policy = OMC_SEM_REFERENCE /
 *   OMC_SEM_TEXTBOOK / OMC_SEM_TWO_PASS: the fits omc_lsm_poly makes with that semantics on the index matrix that
 *   omc_price_american_basket's generator writes for p at (p->seed, p->stream, p->pair_offset); OMC_POLICY_GIVEN: `betas`.
 *   Decisions come from the stored-path exercise tables, on irregular dates from the float64 rule: the same decisions.
 * Paths: every spot is the basket generator's (the section above): asset k of generator pair g draws the vanilla normals at
 *   pair index g + ((uint64_t)k << 40), the correlated normals accumulate with k ascending in the same fmaf chain, the step
 *   is s_k *= exp2(fmaf(+-b_k, y_k, a_k)), the index is formed from the asset spots by the kind's float32 rule.
 * Lower bound: pairs 0 .. n_lower/2 - 1 of stream_lower (pair_offset 0): the index rows are bit for bit the S_keep of
 *   omc_price_american_basket(n_paths = n_lower, stream = stream_lower, pair_offset = 0); each partner stops at the first
 *   date the rule fires; the standard error comes from pair means.
 * Outer paths: that generator at stream_outer, pair_offset 0, n_paths = n_outer: the index matrix [N+1][n_outer] and the
 *   asset matrices A_k [N+1][n_outer] (S_keep and assets_keep of such a call).
 * Inner simulations: inner pair j of item (i, t) is generator pair gbase + j on stream_inner, gbase = (i (N+1) + t)
 *   n_inner/2, started at the outer ASSET spots A_k[t][i]; inner step n consumes generator row n - 1.  The inner index
 *   spots are bit for bit rows 0 .. N-t of the S_keep that omc_price_american_basket writes for b with S0[k] = A_k[t][i],
 *   n_paths = n_inner, stream = stream_inner, pair_offset = gbase and the same T, n_steps, K, weights and rho.
 * Q^, L^, M^, the samples, upper, se_*, ci_*, n_exercised_lower and ms_* are omc_price_american_bounds' with X in the
 *   place of S.  inner_path_steps counts PATH steps (a step of all d assets of one inner path is one).  The inner
 *   simulations run as launches of at most 2^30 / d worst-case inner path steps.  float64 sums in a fixed order: identical
 *   calls return identical bits.
 * With d = 1, w[0] = 1 and q[0] = 0 (arithmetic, best-of or worst-of) every output has the bits of
 *   omc_price_american_bounds for (S0[0], sigma[0]); with d = 1 and a yield q[0] these are the bounds of a single asset
 *   with a continuous dividend yield.  A geometric index is one GBM: price it with d = 1 from (G0, sigma_G, q_G) of
 *   omc_basket_table and w = 1 (kind OMC_BASKET_GEOMETRIC is refused here).
 * The Asian kinds: X is the running average, and the Markov state of a path is its asset spots AND
 *   its running state c_t (l_t).  The outer generator stores that state in a matrix of its own, [N+1][n_outer] beside the
 *   outer asset matrices (row 0 = 0); the inner pairs of item (i, t) start at (A_k[t][i], c_t[i]) and inner step n forms
 *   X_{t+n} by the rule of step t + n: c += B, X = c * (1.0f / (float)(t + n)).  The state is the stored one, never X_t t.
 *   The inner index spots of the arithmetic kind are bit for bit the rule continued in float32 from c_t[i] over the basket
 *   values of the restart call above (kind OMC_BASKET_ARITHMETIC at S0[k] = A_k[t][i]).  The policy sees the average alone.
 * Errors (nothing is launched): -7 null cfg / out; omc_price_american_basket's own (-7, -12, -29 .. -33, the omc_params
 * checks, -24, -11); -34 kind OMC_BASKET_GEOMETRIC; -10 a distributed context; then -4, -7 (betas NULL with
 * OMC_POLICY_GIVEN), -3 and -16 as omc_price_american_bounds; then -38 while option "bounds_exercise_every" holds k >= 2 (no
 * exercise schedule for the index of several assets, the Asian kinds included; with the option back at 0 the call is as above). */
typedef struct {
    omc_bounds bounds;
    double index0;          /* the index of the initial spots, float64 (x0 of omc_basket_table) */
    int32_t n_assets, kind;
} omc_basket_bounds;
int omc_price_american_basket_bounds(omc_ctx* ctx, const omc_params* p, const omc_basket* b, const omc_bounds_config* cfg,
                                     const double* betas /* policy == OMC_POLICY_GIVEN: host [N+1][4] */,
                                     double* betas_out, double* q_out /* NULL or host [n_outer][N] */,
                                     double* samples_out /* NULL or host [n_outer] */, omc_basket_bounds* out);

/* ---- ... with a policy on the index and the runner-up ------------------------------------- */
/* omc_price_american_basket_bounds' game, paths, estimators and outputs (the section above, word for word: Z_t, the Philox
 * coordinates of the lower, outer and inner paths, Q^, L^, M^, the samples, the standard errors from pair means,
 * inner_path_steps, the launches of at most 2^30 / d worst-case inner path steps) with a second policy family: a rule on TWO
 * regressors, the index and the runner-up.  The lower bound of a best-of option is the only out-of-sample price of such a
 * product, and the index alone leaves it percent short; which asset is second closes most of that.
 * Products: OMC_BASKET_BEST_OF and OMC_BASKET_WORST_OF with 2 <= d <= 8.
 * Regressors: v_k = w_k * s_k, the float32 product the index rule forms.  X = the index (max or min of the v_k, the bits
 *   of the generator's index matrix).  Y = the second order statistic of the v_k in the same direction -- second largest for
 *   best-of, second smallest for worst-of --, counted with multiplicity: Y = X when two assets tie.  Y is a value, so no
 *   evaluation order changes it.  u = fma((double)X, 1/K, -1), w = fma((double)Y, 1/K, -1).
 * Policy table: betas [N+1][8] = (c0, c1, c2, c3, c4, c5, n, 0) per date,
 *     cont = fma(w, fma(w, c4, fma(u, c5, c3)), fma(u, fma(u, c2, c1), c0))     = c0 + c1 u + c2 u^2 + c3 w + c4 w^2 + c5 u w
 *   At 1 <= t < N a path exercises iff n_t > 0.5, imm = phi(X) > 0 and imm > cont, all in float64; at N it takes its payoff.
 *   There are no float32 exercise tables (the rule is two-dimensional): option "pass2_tables_irregular_every" has no effect.
 *   With c3 = c4 = c5 = 0 the rule is omc_price_american_basket_bounds' with (c0, c1, c2, n), and so is every output bit.
 * cfg->policy = OMC_SEM_TEXTBOOK: fitted here by classic Longstaff-Schwartz on the p->n_paths paths of the basket generator
 *   at (p->seed, p->stream, p->pair_offset), index and assets kept.  Per-path state (x_ex, tex), initialised to (X_N, N).
 *   For t = N-1 .. 1: the regression set is the paths with phi(X_t) > 0, the target y = D[tex - t] max(phi(x_ex), 0)
 *   (D[k] = exp(-r dt k)), the features f = (u, u^2, w, w^2, uw) of (X_t, Y_t).  The sums n, sum f, sum f f', sum y,
 *   sum f y (27 numbers) are float64 in a fixed order.  The centred system C = sum f f' - sum f sum f' / n,
 *   c = sum f y - sum f sum y / n is solved by LDL' without pivoting in the order of f; feature j (counted from 0) and
 *   every later one get coefficient 0 when n < j + 1.5 or the pivot is not above 1e-12 |C_jj| + 1e-300;
 *   c0 = ybar - sum c_k fbar_k, n_t = n (a date with n < 0.5 gets a row of zeros: nobody exercises there).  Every path,
 *   in the set or not, then applies the rule of date t and updates (x_ex, tex).  n_0 = n_N = 0.
 * cfg->policy = OMC_POLICY_GIVEN: the caller's table `betas`, host [N+1][8].  betas_out: NULL or host [N+1][8].
 * Errors (nothing is launched): omc_price_american_basket_bounds' own, and -35 kind OMC_BASKET_ARITHMETIC or one asset
 * (OMC_BASKET_GEOMETRIC keeps -34); -4 also for OMC_SEM_REFERENCE and OMC_SEM_TWO_PASS; -16 also for more than 512 dates
 * (the kernels keep the policy rows, 64 bytes per date, in LDS; omc_price_american_basket_bounds has no such cap); -38, after
 * all of these, while option "bounds_exercise_every" holds k >= 2.
 * The Asian kinds, any d in 1 .. 8: the second regressor is the current basket value, Y = B_t, where
 *   best-of and worst-of use the runner-up: the Markov state of the option is (average, spot), and the average alone leaves
 *   the lower bound percent short.  The same table, the same rule on (u, w) with w = fma((double)B, 1/K, -1), the same fit,
 *   solve, truncation rule and 512-date cap; paths, running state and inner starts as omc_price_american_basket_bounds has
 *   them for these kinds.  -35 does not apply to them.
 * Memory: the fit keeps the asset matrices of its paths, n_assets (N+1) n_paths floats on the device; a request the card
 * cannot hold fails as a HIP allocation error (a positive code), as for every workspace of the library. */
int omc_price_american_basket_bounds_runnerup(omc_ctx* ctx, const omc_params* p, const omc_basket* b,
                                              const omc_bounds_config* cfg,
                                              const double* betas /* policy == OMC_POLICY_GIVEN: host [N+1][8] */,
                                              double* betas_out /* NULL or host [N+1][8] */,
                                              double* q_out /* NULL or host [n_outer][N] */,
                                              double* samples_out /* NULL or host [n_outer] */, omc_basket_bounds* out);

/* ---- Andersen-Broadie price bounds for American options under Heston ---------------------- */
/* omc_price_american_bounds for p->model = OMC_MODEL_HESTON, scheme OMC_HESTON_REFERENCE_CLAMP or
 * OMC_HESTON_FULL_TRUNCATION: the same game Z_t = exp(-r t dt) max(phi(S_t), 0), t = 1..N, the same policy table betas
 * [N+1][4], stopping rule, estimators, outputs, argument list and result struct (the section "price bounds for American
 * options" above, word for word, with the Heston generator in the place of the GBM one).  One GPU.
 * What the policy sees: the SPOT alone.  The fitted policies are omc_lsm_poly's fits on the Heston paths of p
 *   (omc_heston_paths_f32 at p->seed, p->stream, p->pair_offset); the variance is not a regressor.
 * What the bounds bound: the Bermudan game of the DISCRETISED scheme on the grid -- the Markov chain (S_t, V_t) that
 *   heston_scheme defines with n_steps steps, exercisable at every step -- not the continuous-time Heston model and not the
 *   continuously exercisable option.  lower is what the spot-only policy earns in that game; upper bounds the value under
 *   ANY policy, one that sees the variance included: upper - lower contains what the spot-only policy gives away.
 * Lower bound: the n_lower paths of omc_heston_paths_f32(n_lower, N, .., seed, stream_lower, pair_offset 0, scheme), bit
 *   for bit; each partner of a pair stops at the first date the rule fires on its spot.
 * Outer paths: omc_heston_paths_sv_f32(n_outer, N, .., seed, stream_outer, 0, scheme): S_t[i] and the variance state
 *   V_t[i].  The martingale needs the conditional expectation given the whole Markov state, so inner pair j of item
 *   (i, t) starts BOTH partners at (S_t[i], V_t[i]); it is generator pair g = (i (N+1) + t) (n_inner/2) + j of stream
 *   stream_inner, and inner step k = 1..N-t consumes that pair's Heston step k: rows 2(k-1) and 2(k-1)+1 of
 *   omc_gbm_normals_f32(.., 2 N, seed, stream_inner, pair_offset g) as (z1, z2), the partner (-z1, -z2).  The inner spots
 *   are bit for bit omc_heston_paths_from_normals_f32(z1, z2, S0 = S_t[i], v0 = V_t[i], ..) (a float32 is exact in the
 *   double argument; that entry point takes a negative v0 of scheme 1 as it is).
 * Q^, L^, M^, the samples, upper, se_*, ci_*, n_exercised_lower, inner_path_steps and ms_* as omc_price_american_bounds.
 *   A step draws two normals, so the inner simulations run as launches of at most 2^29 worst-case inner path steps.
 *   Option "pass2_tables_irregular_every" acts as there.  float64 sums in a fixed order: identical calls return identical
 *   bits.
 * Errors (nothing is launched): -7 null cfg / out; the omc_params checks; -12 p->model not OMC_MODEL_HESTON, or
 * heston_scheme OMC_HESTON_CALIBRATOR (its arithmetic Euler step lets the spot cross zero) or OMC_HESTON_QE (no bounds
 * kernels are built for it); then -10, -4, -7, -3, -16 as
 * omc_price_american_bounds, which itself keeps refusing Heston with -12.
 * Option "bounds_exercise_every" = k >= 2 (an exercise schedule; "... with an exercise schedule" above, word for word, with the
 *   inner pairs started at the outer (S, V) state at tau_j and the fit on the gathered Heston paths): taken with
 *   cfg->regressors = OMC_HESTON_REG_SPOT, schemes 0 and 1; it changes the game, not a route.  On a fine grid it bounds the
 *   option exercisable at the scheduled dates of the discretised scheme without inner simulations at every step.
 *
 * ---- ... with a policy on the spot and the variance state ----
 * Selector: cfg->regressors = OMC_HESTON_REG_SPOT (0): everything above, bit for bit.  OMC_HESTON_REG_SPOT_VARIANCE (1): a
 *   second policy family, a rule on TWO regressors.  Under Heston the variance is half of the Markov state; the spot-only
 *   rule is the one simplification the lower bound above still carries.  Any other value is refused with -4.  The field is
 *   omc_bounds_config's former reserved one: no new entry point, the same struct layout, OMC_ABI_VERSION unchanged;
 *   omc_price_american_bounds, omc_price_american_basket_bounds and omc_price_american_basket_bounds_runnerup ignore it.
 * Regressors: X = the float32 spot.  Y = the float32 variance state as the scheme's step leaves it -- the value
 *   omc_heston_paths_sv_f32 stores: scheme OMC_HESTON_REFERENCE_CLAMP floored at 0, OMC_HESTON_FULL_TRUNCATION unfloored,
 *   negative values included.  u = fma((double)X, 1/K, -1), w = fma((double)Y, 1/vbar, -1) with vbar = max(v0, theta) in
 *   double.  vbar is a scale for conditioning only, not a model quantity: a caller who builds a `given` table must form w
 *   with the same vbar.
 * Policy table: betas [N+1][8] = (c0, c1, c2, c3, c4, c5, n, 0) per date,
 *     cont = fma(w, fma(w, c4, fma(u, c5, c3)), fma(u, fma(u, c2, c1), c0))     = c0 + c1 u + c2 u^2 + c3 w + c4 w^2 + c5 u w
 *   At 1 <= t < N a path exercises iff n_t > 0.5, imm = phi(X) > 0 and imm > cont, all in float64; at N it takes its payoff:
 *   omc_price_american_basket_bounds_runnerup's rule and row layout with the variance in the runner-up's place.  There are
 *   no float32 exercise tables: option "pass2_tables_irregular_every" has no effect.  With c3 = c4 = c5 = 0 every output has
 *   the bits of the spot-only call given (c0, c1, c2, n).
 * cfg->policy = OMC_SEM_TEXTBOOK: fitted here by classic Longstaff-Schwartz on the p->n_paths paths of
 *   omc_heston_paths_sv_f32 at (p->seed, p->stream, p->pair_offset), spots and variance state kept.  Per-path state
 *   (x_ex, tex), initialised to (S_N, N).  For t = N-1 .. 1: the regression set is the paths with phi(S_t) > 0, the target
 *   y = D[tex - t] max(phi(x_ex), 0), the features f = (u, u^2, w, w^2, uw) of (S_t, V_t); the 27 float64 sums in a fixed
 *   order, the centred 5 x 5 system by LDL' without pivoting and the truncation rule (feature j and every later one get
 *   coefficient 0 when n < j + 1.5 or the pivot is not above 1e-12 |C_jj| + 1e-300) are those of the runner-up section,
 *   word for word; n_0 = n_N = 0.  With xi = 0 and v0 = theta exact in float32, w is 0 on every path and the rule gives
 *   c3 = c4 = c5 = 0 exactly.
 * cfg->policy = OMC_POLICY_GIVEN: the caller's table `betas`, host [N+1][8].  betas_out: NULL or host [N+1][8].
 * Everything else is unchanged: the game, the discretised scheme as the model, the Philox coordinates of the lower, outer and
 *   inner paths, inner pairs started at (S_t[i], V_t[i]), Q^, L^, M^, the samples, the standard errors from pair means,
 *   inner_path_steps, the launches of at most 2^29 worst-case inner path steps, the refusals -3, -7, -10, -12, -16.
 * Errors, beside those: -4 a selector other than 0 or 1, or OMC_SEM_REFERENCE / OMC_SEM_TWO_PASS with selector 1; -5
 *   max(v0, theta) not above 0; -16 more than 512 dates (the kernels keep the policy rows, 64 bytes per date, in LDS);
 *   -38, after all of these, while option "bounds_exercise_every" holds k >= 2 (selector 1 takes no exercise schedule).
 * Memory: the fit additionally keeps the variance state V [N+1][ld] of its fitting paths on the device. */
enum { OMC_HESTON_REG_SPOT = 0, OMC_HESTON_REG_SPOT_VARIANCE = 1 };
int omc_price_american_bounds_heston(omc_ctx* ctx, const omc_params* p, const omc_bounds_config* cfg,
                                     const double* betas /* policy == OMC_POLICY_GIVEN: host [N+1][4], or [N+1][8] */,
                                     double* betas_out, double* q_out /* NULL or host [n_outer][N] */,
                                     double* samples_out /* NULL or host [n_outer] */, omc_bounds* out);

/* ---- Andersen-Broadie price bounds under jump-diffusion: Merton and Bates ------------------ */
/* The jump generator as an entry point and the price bounds with the jump law are declared, with their contract, in
 * include/omc_jump_bounds.h, which includes this header: this file's set of entry points is unchanged. */

/* ---- calibrator inner loop -------------------------------------- */
/* replaces HestonPricer.price_options_batch / price_european_option
 * (options_model_3/heston_calibration.py:259-312) for ONE expiry: simulate n_paths antithetic
 * Heston paths (terminal spots only, no path matrix), then the discounted mean payoff of every
 * strike.  strikes / prices / stderrs are host arrays of n_strikes (stderrs may be NULL). */
int omc_heston_price_strikes(omc_ctx* ctx, int64_t n_paths, int n_steps, double S0, double r,
                             double T, double v0, double kappa, double theta, double xi, double rho,
                             uint64_t seed, uint64_t stream, int scheme, const double* strikes,
                             int n_strikes, int is_put, double* prices, double* stderrs);
/* the same for a whole quote SURFACE -- what ONE evaluation of the calibrator's objective asks for
 * (heston_calibration.py:283-312 loops `for T in unique_T`; :404-472 calls it once per optimizer iteration): n_expiries
 * expiries (host, expiries[e] > 0) each simulated on its own Philox sub-stream streams[e] (host), n_quotes quotes with
 * strike strikes[q] on expiry expiry_of[q] (host int32, 0 .. n_expiries-1).  One launch for all simulations (expiry on
 * grid.y), one for all quotes, one table upload, one read-back, one wait.  Every quote has the bits of its own
 * omc_heston_price_strikes(T = expiries[expiry_of[q]], stream = streams[expiry_of[q]], strike = strikes[q]) call. */
int omc_heston_price_surface(omc_ctx* ctx, int64_t n_paths, int n_steps, double S0, double r, double v0, double kappa,
                             double theta, double xi, double rho, uint64_t seed, int scheme, const double* expiries,
                             const uint64_t* streams, int n_expiries, const double* strikes, const int32_t* expiry_of,
                             int n_quotes, int is_put, double* prices, double* stderrs);

/* ---- NN continuation-value regressor: fused training of the network ------------------------ */
/* replaces the minibatch loop of price_american_enhanced_lsm (options_model_3.py:565-600:
 * SingleLSMNet(7, hidden, layers) :85-103, nn.MSELoss, optim.Adam(lr, weight_decay), shuffled
 * minibatches) for hidden = 32, 64 or 128 with layers = 2 (BASELINE config 5 names 7 -> 64 -> 64 -> 1)
 * or 3 (the depth SingleLSMNet always has in the reference; 3 x 128 is its default) -- see
 * omc_mlp_train_supported for the batch sizes; anything else returns -9.
 * One call = one epoch over `n_rows` rows of
 * `data` ([n_rows][8] float32 device memory: 7 normalised features + normalised target):
 * ceil(n_rows / batch) optimizer steps of float32 MFMA forward/backward + Adam.  The epoch
 * visits the rows in a pseudo-random permutation keyed by `shuffle_key` (a Feistel network with
 * cycle-walking, evaluated in the kernel: no randperm, no gather; 0 = storage order) --
 * omc_mlp_shuffle_indices writes that permutation out (out[i] = row visited at position i).
 * `params` (device, omc_mlp_param_count floats) is laid out W1|b1 as [hidden][8] (bias in
 * column 7), then per further hidden layer W [hidden][hidden] and b [hidden], then the output
 * weights [hidden] and bias [1]; adam_m / adam_v are the moment buffers (zero
 * them before the first epoch); *step counts optimizer steps across calls (bias correction).
 * dropout is applied after each ReLU as in training mode (Philox bits keyed by `seed`).
 * *mean_loss = mean over the epoch's steps of the batch-mean squared error (the value the
 * reference feeds to ReduceLROnPlateau and its early-stopping test, :601-613). */
int omc_mlp_param_count(int hidden, int layers);
/* Pass 2 of the NN flow (options_model_3.py:615-651): sticky backward sweep over a device path
 * matrix with the trained network as continuation value -- features [1, x, x^2, x^3,
 * max(x-1,0), s, x*s] of x = S/K normalised with (feat_mean, feat_std) (host, 7 each), network
 * output scaled back by y_std, y_mean; exercise where payoff > continuation; dropout (> 0) stays
 * active as in the reference, which never calls .eval() on this net; cash-flows valued at
 * t = dt.  Networks: SingleLSMNet(7, hidden, layers) with hidden in {64, 128} and layers in
 * {2, 3} -- the reference's default is (128, 3), options_model_3.py:87 -- anything else: -9.
 * params (device, omc_mlp_param_count(hidden, layers) floats): W1|b1 as [hidden][8] (bias in
 * column 7), then per further hidden layer W [hidden][hidden] and b [hidden], then the output
 * weights [hidden] and bias [1]; for (64, 2) this is omc_mlp_train_epoch's layout.
 * Optional sx_out / tex_out (host). */
int omc_lsm_apply_mlp(omc_ctx* ctx, const float* S, int64_t ld, int64_t n_paths, int n_steps, double K,
                      double r, double T, int is_put, int hidden, int layers, const float* params,
                      const double* feat_mean, const double* feat_std, double y_mean, double y_std,
                      double dropout, uint64_t seed, omc_result* res, float* sx_out, int32_t* tex_out);
/* the same on one rank's shard of a job: the dropout key of column j is its column in the UNSHARDED matrix,
 * j + col_base0 for the first half of this matrix's columns (first partners) and j - n_paths / 2 + col_base1 for the
 * second -- (pair_offset, P_global + pair_offset) -- so a shard draws the masks the single GPU draws.  The sums in
 * `res` are the shard's; the caller adds them over the ranks. */
int omc_lsm_apply_mlp_shard(omc_ctx* ctx, const float* S, int64_t ld, int64_t n_paths, int n_steps, double K,
                      double r, double T, int is_put, int hidden, int layers, const float* params,
                      const double* feat_mean, const double* feat_std, double y_mean, double y_std,
                      double dropout, uint64_t seed, omc_result* res, float* sx_out, int32_t* tex_out,
                            int64_t col_base0, int64_t col_base1);
/* Pass 1 of the NN flow (options_model_3.py:482-563) straight from a device path matrix: every
 * in-the-money (step, path), steps N-1 down to 1 and paths ascending within a step (the reference's
 * order), becomes one row of `data` ([rows][8] float32, device): the 7 features [1, x, x^2, x^3,
 * max(x-1,0), s, x*s] of x = S/K, s = sqrt(max(T - t dt, 1e-6)), normalised by their means and
 * population stds over all rows (zero std -> 1), and the target (terminal payoff discounted to t)
 * normalised likewise.  *n_rows = number of rows; with data == NULL only the count is made (call
 * once to size the buffer, then again with data and cap_rows >= *n_rows).  stats16 (host) =
 * feat_mean[7], feat_std[7], y_mean, y_std -- on a context with a communicator / hook those of ALL ranks' rows (see the
 * sharded NN regressor below); every rank of the job must then make the call, also one without any row.  There the
 * call with `data` is COLLECTIVE (two all-reduces of 9 and 8 doubles): a failure only one rank can see (its row buffer
 * too small, no memory for its scratch) travels as a flag in the first of them and EVERY rank returns an error -- the
 * rank's own, 3102 on its peers -- instead of leaving them inside a collective; a job without any in-the-money row
 * returns the default statistics (means 0, stds 1) on every rank.
 * S is read twice IN ALL: one sweep counts the rows of every (step, 256-path tile) and forms the statistics -- power sums
 * around a workgroup's first row (a real row: a column that is constant has deviation 0 exactly), added over its lanes
 * in a fixed order, turned into (n, mean, M2) triples per workgroup and merged by Chan's formula in a fixed two-level
 * tree: the two-pass values of :550-563 to ~1e-14, a constant column's variance exactly 0 -- and one sweep writes the
 * rows (records staged through LDS, contiguous 16-byte stores).  The count call (data == NULL) makes the first sweep and leaves its results in the context; the call with `data`
 * starts from them when it is the NEXT call on this context with the same arguments and S has not been written in
 * between (any other call on the context drops them, and the call with `data` then sweeps again itself). */
int omc_nn_build_rows(omc_ctx* ctx, const float* S, int64_t ld, int64_t n_paths, int n_steps, double K,
                      double r, double T, int is_put, float* data, int64_t cap_rows, int64_t* n_rows,
                      double* stats16);
/* Regressor "ols7": the v3 two-pass flow (options_model_3.py:482-516 pass 1, :542-563 normalisation, :615-651 pass 2,
 * :651 mean at t = dt) with ONE global least-squares fit on the reference's seven features [1, x, x^2, x^3, max(x-1,0),
 * s, x*s] (create_regression_features, :105-121) in place of the network -- the reference validates `lsm_poly_degree`
 * and never uses it; this is the linear regressor its own features define, between the per-step 3-term
 * polynomial (omc_lsm_poly) and the network.  Pass 1 is one sweep over S (co-moments of the 6 non-constant features and
 * the target -- accumulated for u = x - 1, the same span in a better conditioned basis --, float64, merged by Chan's
 * formula in a fixed order); the fit is lstsq on the normalised design matrix
 * (zero-variance columns get weight 0, as numpy's minimum-norm solution gives them); pass 2 applies it, strict >, sticky.
 * res->sum_nitm = rows of the regression; weights7 (host, may be NULL) = the fit, column 0 the constant; stats16 (host,
 * may be NULL) = feat_mean[7], feat_std[7], y_mean, y_std as omc_nn_build_rows returns them.  On a context with a
 * communicator / hook the call is collective: the fit is over ALL ranks' rows (two all-reduces of 9 and 28 doubles merge the
 * ranks' co-moments, one of 8 the result sums) and `res` is the job's; a failure only one rank can see (no memory for its
 * path matrix -- omc_price_american_ols7's largest allocation -- or workspace, a HIP error in its sweep: the ninth double
 * of the first all-reduce; a HIP error in its pass 2: slot 7 of the result sums, which the kernels leave at zero) travels
 * as a flag and EVERY rank returns an error -- the rank's own, 3103 on its peers -- instead of leaving them inside a
 * collective.  No allocation stands between a rank and a collective its peers have entered: the few hundred bytes the
 * flags travel through exist from omc_comm_init / omc_set_allreduce_hook on. */
int omc_lsm_ols7(omc_ctx* ctx, const float* S, int64_t ld, int64_t n_paths, int n_steps, double K, double r, double T,
                 int is_put, omc_result* res, double* weights7, double* stats16, float* sx_out, int32_t* tex_out);
/* the same as one fused call (paths into the context's own matrix, then omc_lsm_ols7): the facade's regressor="ols7" */
int omc_price_american_ols7(omc_ctx* ctx, const omc_params* p, omc_result* res, double* weights7, double* stats16);
/* Normalisers of the training rows (options_model_3.py:550-563) in float64: for rows i < n_rows
 * with x[i] = S/K, step index t[i] and target y[i] (device arrays), out16[0..6] = means of
 * [x, x^2, x^3, max(x-1,0), s, x*s, y] with s = sqrt(max(T - t*dt, 1e-6)), out16[8..14] =
 * their population variances (two passes: mean first, then squared deviations).  out16: host. */
int omc_nn_feature_stats(omc_ctx* ctx, const double* x, const int32_t* t, const double* y,
                         int64_t n_rows, double T, double dt, double* out16);
/* 1 if omc_mlp_train_epoch covers this network shape at this minibatch size: hidden 32, 64 or 128 (the
 * reference's default width) with 2 or 3 hidden layers, any batch (32 is also the width the per-step ContNet flow
 * trains at, omc_lsm_contnet).  Wider networks (256 units: a connection's operands no longer fit the registers /
 * LDS the kernels keep them in) train and sweep through PyTorch-ROCm, with a RuntimeWarning from nn_regressor. */
int omc_mlp_train_supported(int hidden, int layers, int64_t batch);
int omc_mlp_train_epoch(omc_ctx* ctx, const float* data, int64_t n_rows, int64_t batch, int hidden,
                        int layers, float* params, float* adam_m, float* adam_v, int64_t* step,
                        double lr, double beta1, double beta2, double eps, double weight_decay,
                        double dropout, uint64_t seed, uint64_t shuffle_key, double* mean_loss);
int omc_mlp_shuffle_indices(omc_ctx* ctx, int64_t n_rows, uint64_t shuffle_key, int64_t* out_device);
/* Which of the four trainer kernels omc_mlp_train_epoch runs for this shape at this minibatch size: 1 = one
 * workgroup per 128 rows with the weights in LDS (64 units, more than 32 tiles of 32 rows), 2 = one 32-row tile per
 * wave, 3 = one 32-row tile per workgroup, 4 = one 16-row tile per workgroup (minibatches of up to 4,096 rows: the
 * reference's own min(256, R)), 0 = not covered.  The kernels hold the hidden units in different register orders, so
 * WHICH units dropout drops for a given (seed, step, row) depends on it. */
int omc_mlp_train_variant(int hidden, int layers, int64_t batch);
/* Inspection: the dropout masks themselves.  nn.Dropout's random stream in the reference is torch's global generator
 * (options_model_3.py:455, 85-103); here a unit's 16 random bits come from Philox4x32-10 keyed by `seed` with counter
 * (row key, step, layer / half-tile tag, constant), stretched by a multiply-with-carry stream (csrc/omc_mlp_dev.h
 * relu_dropout).  out (host, [layers][n_rows][hidden] bytes): 1 = kept, 0 = dropped, as kernel `variant` draws them
 * (0 = pass 2, omc_lsm_apply_mlp: row key = path column, step = time step t; 1 .. 4 = omc_mlp_train_variant: row key
 * = position in the minibatch, step = optimizer step counted from 1).  keys (host, n_rows, may be NULL = 0, 1, 2, ...).
 * oracle/dropout.py restates the definition in numpy; tests compare the two bit for bit and then compare training and
 * pass 2 with the float32 / float64 restatement of the reference's arithmetic under these masks. */
int omc_mlp_dropout_masks(omc_ctx* ctx, int variant, int hidden, int layers, int64_t n_rows, const uint32_t* keys,
                          uint32_t step, uint64_t seed, double dropout, uint8_t* out);

/* ---- the NN regressor sharded over the ranks of a job (options_model_3.py:542-613) ---------
 * The reference trains ONE network on the rows of ALL paths.  With the paths sharded by antithetic pair, every rank
 * builds the rows of its own paths and the job trains the network the single GPU would train:
 *   1. omc_nn_build_rows on a context with a communicator / hook: the normalisers are those of ALL ranks' rows (row
 *      count, sums and squared deviations from the global means all-reduced: 3 x 8 doubles); *n_rows stays the rank's
 *      own count and `data` its own rows.
 *   2. The job's rows in the reference's order (step N-1 .. 1, global column ascending) are the concatenation of
 *      segments (step, half, rank) -- a rank's matrix holds its pairs' first partners in columns [0, P_local) and the
 *      second partners behind them, the global matrix all ranks' first partners, then all second partners.
 *      omc_nn_half_counts returns a rank's segment sizes ([n_steps - 1][2] int64 on the host, index n_steps - 1 - t);
 *      the ranks exchange them (omc_comm_allreduce_f64 of a zero-padded table) and build gstart[nseg + 1] (global index
 *      of each segment's first row, ascending, gstart[nseg] = rows_global) and lstart[nseg] (where the segment starts
 *      among the rank's own rows, -1 for another rank's) -- options_model_amd/nn_dist.py: segment_tables.
 *   3. Per epoch, omc_mlp_shard_epoch evaluates the single-GPU trainer's keyed permutation over rows_global, keeps the
 *      positions whose row this rank owns (ascending), gathers those rows into data_epoch ([n_rows_local][8] float32,
 *      device), their positions inside their minibatch into drop_pos (device uint32: the dropout key, so every rank
 *      draws the masks of the unsharded run) and returns step_off (HOST int64 [steps + 1], steps = ceil(rows_global /
 *      batch)): minibatch k holds this rank's rows [step_off[k], step_off[k + 1]) of data_epoch.
 *   4. omc_mlp_train_epoch_sharded runs the epoch: forward / backward over the rank's part of each minibatch, scaled
 *      by the GLOBAL minibatch size; the gradient sums and the loss sum (parameter count + 1 doubles) are all-reduced
 *      on the context's stream; every rank applies the same Adam step, so the parameters stay identical on all ranks
 *      and equal those of the single-GPU run up to float32 summation order.  *mean_loss is the job's.
 * Pass 2 (omc_lsm_apply_mlp) is local; its sums are added over the ranks by the caller. */
int omc_nn_half_counts(omc_ctx* ctx, const float* S, int64_t ld, int64_t n_paths, int n_steps, double K, int is_put,
                       int64_t* counts /* host [(n_steps - 1)][2] */);
int omc_mlp_shard_epoch(omc_ctx* ctx, const float* data, int64_t n_rows_local, int64_t rows_global, int64_t batch,
                        uint64_t shuffle_key, const int64_t* gstart, const int64_t* lstart, int nseg,
                        int segs_per_step /* 2 x ranks: lets the kernel search the table in two levels; 0 = unknown */,
                        float* data_epoch, uint32_t* drop_pos, int64_t* step_off);
int omc_mlp_train_epoch_sharded(omc_ctx* ctx, const float* data_epoch, int64_t n_rows_local, int64_t rows_global,
                                int64_t batch, int hidden, int layers, float* params, float* adam_m, float* adam_v,
                                int64_t* step, double lr, double beta1, double beta2, double eps, double weight_decay,
                                double dropout, uint64_t seed, const int64_t* step_off, const uint32_t* drop_pos,
                                double* mean_loss);

/* ---- local-vol paths through the implied-vol network ------------------------ */
/* replaces simulate_local_vol_paths_antithetic (options_model_3.py:300-333) together with the
 * IVModel.get_volatility_batch call it makes every step (:263-298): S_t = S_{t-1} exp((r -
 * sigma^2/2) dt + sigma sqrt(dt) z) with sigma = ImprovedIVNetwork(log(K/S)/m_scale, tau/tau_scale)
 * (NN_training_stock_iv.py:109-155; hidden_dim 64, `layers` residual LayerNorm/GELU blocks),
 * clamped at `epsilon` and 1e-6, evaluated inside the kernel on the matrix cores.  S: device
 * [n_steps+1][ld] float32, antithetic partner of column j is j + n_paths/2; Z: device
 * [n_steps][n_paths/2] float32 normals (omc_gbm_normals_f32 makes them, or inject your own).
 * params (device, omc_localvol_param_count floats): input_proj as [64][4] (w_m, w_tau, bias, 0),
 * per block Linear W [64][64], b [64], LayerNorm gamma [64], beta [64], then output w [64], b. */
int omc_localvol_param_count(int hidden, int layers);
int omc_localvol_paths_f32(omc_ctx* ctx, float* S, int64_t ld, int64_t n_paths, int n_steps, double S0,
                           double r, double T, double K, int hidden, int layers, const float* params,
                           double m_scale, double tau_scale, double epsilon, const float* Z);

/* ---- many small networks trained side by side (curves with the NN regressor) --------------------------------- */
/* The reference prices a value-vs-expiry curve point by point, training a fresh SingleLSMNet per point
 * (compute_curve_for_S0, options_model_3.py:697-713 -> :565-613); at its minibatch of 256 rows one network occupies
 * 8 of the chip's 256 CUs.  This trains n networks of ONE shape (hidden x layers) for one epoch each, side by side:
 * one launch pair per optimizer step for all of them (problem index on the grid), each network on its own rows,
 * learning rate, dropout / shuffle keys and step counter.  Every network ends the epoch with exactly the parameters,
 * Adam moments and mean loss that its own omc_mlp_train_epoch call produces (same kernel body, same reductions).
 * jobs[i].step is advanced by the epoch's steps, jobs[i].mean_loss receives the epoch-mean batch loss.  Pointers are
 * device pointers as in omc_mlp_train_epoch.  Shapes: 32 | 64 | 128 units x 2 | 3 hidden layers at
 * minibatches of at most 8192 rows. */
typedef struct {
    const float* data;     /* [n_rows][8] float32: 7 normalised features + normalised target        */
    int64_t n_rows, batch;
    float* params;         /* omc_mlp_param_count(hidden, layers) floats, updated in place           */
    float* adam_m;
    float* adam_v;
    int64_t step;          /* in: optimizer steps taken so far; out: + this epoch's                  */
    double lr;
    uint64_t seed;         /* dropout bits                                                          */
    uint64_t shuffle_key;  /* 0: storage order; else this epoch's keyed permutation                 */
    double mean_loss;      /* out                                                                   */
} omc_mlp_job;
int omc_mlp_train_batch_supported(int hidden, int layers, int64_t batch); /* 1: this shape / minibatch is covered */
int omc_mlp_train_epoch_batch(omc_ctx* ctx, omc_mlp_job* jobs, int n, int hidden, int layers, double beta1,
                              double beta2, double eps, double weight_decay, double dropout);

/* ---- a sequence of pricings without host synchronisation in between ------------------------- */
/* n independent pricings enqueued back to back on the context's stream (pricing i + 1 is launched while
 * pricing i runs; every pricing's result sums land in their own slot of a host-mapped buffer; one wait
 * at the end).  res[i] equals what omc_price_american(p[i]) returns, bit for bit; ms_paths / ms_pass1 /
 * ms_pass2 are measured on the first pricing (and on every k-th one with option "seq_event_stride" = k;
 * res[i].timed marks them), ms_total is the average over the sequence.  Across GPUs the
 * moment tables are all-reduced per pricing as usual, but the result sums of all n pricings travel in ONE
 * collective of 8n doubles after the last pricing (the hook is called once with count = 8n); a hook must only
 * ENQUEUE its collective on the stream (as torch.distributed does), then the sequence stays free of host
 * waits across ranks too.  With a native communicator see also option "seq_overlap". */
int omc_price_american_seq(omc_ctx* ctx, const omc_params* p, int n, omc_result* res);
/* Per-step flows (semantics 0 / 1; the kernel of Options_model.py:108-157): a sequence whose pricings share
 * (n_paths, n_steps, r, T, semantics) advances K of them with EVERY launch of the per-timestep kernel -- K path
 * matrices resident, one launch boundary per time step for all K, and across GPUs the K moment vectors of a step in
 * ONE all-reduce of 8K doubles.  One pricing alone is latency-bound (13 MB and ~6 us per launch at 1M paths); K of
 * them fill the chip.  res[i] still carries the bits of omc_price_american(p[i]): the summation tree of a pricing
 * does not depend on K.  Option "seq_step_k": -1 = default (as many as keep one launch within ~200 MB, at most 32:
 * 16 at 1M paths, 32 at 250k), 1 = off, k <= 32; K is further limited by a byte
 * budget for the resident matrices (OMC_SEQ_STEP_BYTES, default 64e9).  This returns the K a sequence would use
 * (1 = one pricing at a time, 0 = invalid arguments). */
int omc_seq_step_width(omc_ctx* ctx, const omc_params* p, int n);
/* Two-pass flow (semantics 2) on one card: a run of consecutive pricings on folded storage with option "pass2_tables"
 * on that share n_paths, n_steps, r, T and the fold constants (S0^2 / K and the drift: one fold table, one discount
 * table; is_put, seed, stream and pair_offset may differ) is priced in GROUPS of K.  Every member keeps its own
 * generator, pass-1 sweep and pass-2 sweep, each a launch of its own and the generator right in front of its pass 1,
 * but the group's K pass-1 reductions, K table builds and K finalizes run as three launches instead of 3K: those are
 * the latency-bound launches of a pricing (46 us of its 362 us of kernel time at 1M paths x 252 steps), during which
 * the chip is nearly empty.  res[i] still carries the bits of omc_price_american(p[i]).  A timed member
 * (res[i].timed) reports ms_pass2 of its pass-2 SWEEP alone; outside a group ms_pass2 includes the table build in
 * front of the sweep.  ms_total and ms_lsm = ms_total - ms_paths are per pricing over the whole sequence as ever, the
 * shared launches inside them.  Every member keeps its path matrix resident until its group ends.
 * Option "seq_two_pass_k": -1 = default (groups of 8; pricings of more than 2^29 path-steps, 2.1M paths x 252 steps,
 * one at a time: groups gain 2 % at 2M paths x 252 steps, nothing at 4M and lose 1 % at 8M), 1 = one pricing at a time (the launch order of omc_price_american), k <= 32; the
 * environment variable OMC_SEQ_TWO_PASS_K sets the same where the option is -1.  K is further limited by the byte
 * budget of the resident matrices (OMC_SEQ_STEP_BYTES, default 64e9, and 80 % of the card's free memory) and halves
 * when an allocation fails.  A context with a communicator or an all-reduce hook, full storage, "pass2_tables" = 0 and
 * every other flow: one pricing at a time, as before.  This returns the K of the run that starts at p[0] (1 = not
 * grouped, 0 = invalid arguments). */
int omc_seq_group_width(omc_ctx* ctx, const omc_params* p, int n);

/* ---- a whole option chain from one set of paths ------------------------------------------- */
/* n quotes of ONE expiry -- strikes and sides in e[], everything else in p (p->K and p->is_put are ignored) -- priced
 * from one generator launch and one path matrix: the paths depend on neither the strike nor the side.  Two-pass flow
 * (p->semantics = OMC_SEM_TWO_PASS), antithetic pairs (p->antithetic = 1), GBM or Heston, one GPU.
 * THE CONTRACT: res[i] equals omc_price_american(ctx, p with K = e[i].K and is_put = e[i].is_put, ...) bit for bit --
 * price, sum, sumsq, std, zero_prob, every count and `folded` -- and slice i of betas_out ([n][n_steps+1][4], host, may
 * be NULL) equals the fits that single call makes (rows 0 and n_steps zero, as omc_price_american_greeks returns them),
 * whatever else the chain holds, in whatever order, whatever omc_chain_width says.  Storage is chosen as by the single
 * call (option "fold_antithetic"); on folded storage every entry has its own fold table cK_j[t] = c0_j g^t.
 * Routes: FUSED (option "chain_fused" = 1; GBM on folded storage with "pass2_tables" on, n_steps >= 2):
 * entries are split by side and into launches of up to omc_chain_width entries whose two sweeps read every stored spot
 * once -- conversion to float64 and the reciprocal behind the partner's moneyness once per spot -- and form every
 * entry's sums in the tile, block and slot geometry of the single kernels; UNFUSED (Heston, full storage,
 * "pass2_tables" = 0, and the default, "chain_fused" = 0): the single-strike sweeps per entry on the shared matrix.  Either way the
 * pass-1 reductions, table builds and finalizes of up to 16 entries share one launch each.
 * EXERCISE SCHEDULES: e[i].exercise_every = k is the entry's schedule on the grid of n_steps = N dates.
 *   k = 0 or 1   every date: the American quote, THE CONTRACT above.
 *   k >= 2       a Bermudan quote: early exercise only at the dates t in 1 .. N-1 with (N - t) % k == 0 -- the schedule
 *                is anchored at expiry, which takes the payoff as ever; k >= N leaves no early date (the European value
 *                of the flow).  res[i] is the two-pass flow with every other date skipped in BOTH passes: rows of slice
 *                i of betas_out at scheduled dates carry the bits of the American entry's fits of the same (K, is_put),
 *                every other row is zero, sum_nitm sums the scheduled dates, pass 2 is the sticky backward rule over
 *                them, valued as the flow values, exp(-r dt (t - 1)).  The entry's sweeps read its scheduled rows (and
 *                the expiry's) only -- but for pass 1 on full storage when n_paths is a multiple of 4, which walks
 *                all rows to keep the fits' bits.  It changes what no other entry returns; a chain that holds one takes the unfused
 *                route as a whole (info->fused = 0), on which the American entries carry the same bits.
 *   k < 0        refused, -37.
 * Timings: res[i].ms_* repeat the chain's whole-call times, res[i].timed is 1 for i = 0 only; info (may be NULL): the
 * route taken, the number of sweep launches per pass, and the phases -- ms_paths the generator, ms_pass1 the pass-1
 * sweeps + reductions, ms_pass2 the table builds + pass-2 sweeps + finalizes, ms_total from the first launch to the
 * last completion (it also holds the entries' fold tables, which every call builds anew in front of the generator).
 * Errors: those of omc_price_american for p (nothing is launched); -7 null e / res; -3 n < 1 or n > 256; -4 an entry
 * whose K is not finite and positive or whose is_put is not 0 / 1, or p->semantics != 2; -15 p->antithetic == 0;
 * -37 an entry whose exercise_every is negative; -10 a context with a communicator or an all-reduce hook.  They are
 * checked in this order -- p's own, the -4 of every entry, then -37, then -10 -- before anything is launched: res is untouched.
 * Options: "chain_fused" (0 = default: unfused -- 8 quotes at 1M paths x 252 steps in 1.99 ms against 3.08 ms as a
 * sequence; 1 = fused: measured 0.3 - 5.5 % slower than unfused at the sizes of DESIGN.md 13.4, kept as an option), "chain_k" (entries per fused launch at most: -1 = default, 1 .. 16;
 * it can only lower omc_chain_width). */
typedef struct {
    double K;
    int32_t is_put;
    int32_t exercise_every; /* 0 or 1: every date (American); k >= 2: every k-th date counted back from expiry (it was
                               a reserved field that nothing read: callers that zero it keep their results) */
} omc_chain_entry;
typedef struct {
    int32_t folded, fused, n_launch_groups, reserved;
    double ms_paths, ms_pass1, ms_pass2, ms_total;
} omc_chain_info;
#define OMC_CHAIN_MAX 256
int omc_price_american_chain(omc_ctx* ctx, const omc_params* p, const omc_chain_entry* e, int n, omc_result* res,
                             double* betas_out, omc_chain_info* info);
/* entries per fused launch for a chain of n entries like p: 4, 2 or 1 (the fused pass 2 keeps every entry's exercise
 * state in registers and its tables in LDS: 4 up to 4.2M paths, 2 beyond, where a thread takes four columns); 1 also
 * where the chain takes the unfused route; 0 = invalid arguments */
int omc_chain_width(omc_ctx* ctx, const omc_params* p, int n);

/* ---- many small pricings in one go ------------------------------------------------------- */
/* replaces the curve loops compute_curve_for_S0 (options_model_3.py:697-713, Options_model.py:
 * 190-211, options_model_2.py:336-355) and their ProcessPoolExecutor fan-out: n independent
 * problems (each its own S0, T, n_steps, n_paths, seed ...) run as ONE set of launches with
 * the batch index on the grid.  All problems of a call share model, semantics, antithetic and
 * Heston scheme; results are identical to n calls of omc_price_american / omc_price_european -- bit for bit when the
 * batch runs the kernels a single call runs: the 16-byte ones, taken when EVERY member has whole groups of four path
 * pairs (n_paths % 8 == 0 with antithetic pairs, % 4 without); otherwise all members run the scalar kernels, whose sums
 * are formed in another block geometry: the same decisions (exact ties of a handful of paths aside), prices to 1e-12.
 * Members are priced on FULL path storage: a member large enough for a single call to fold it (65,536+ paths, option
 * "fold_antithetic") equals the single call made with that option at 0.
 * Whole-batch kernel times are reported in res[0]. */
int omc_price_american_batch(omc_ctx* ctx, const omc_params* p, int n, omc_result* res);
int omc_price_european_batch(omc_ctx* ctx, const omc_params* p, int n, omc_result* res);
/* The same for the regressor the v1 / v2 pricers really run (omc_price_american_contnet: a fresh ContNet per time
 * step): n pricings, problem index on the grid for the whole chain (regression set -> rows -> fresh net -> nn_epochs
 * full-batch Adam steps -> continuation values -> decision), the set sizes never leave the device, no host
 * read-back between the first and the last launch.  nn_seeds[i] keys problem i's nets.  res[i] equals
 * omc_price_american_contnet(p[i], ..., nn_seeds[i]) bit for bit. */
int omc_price_american_contnet_batch(omc_ctx* ctx, const omc_params* p, int n, int nn_hidden, int nn_epochs,
                                     double nn_lr, const uint64_t* nn_seeds, omc_result* res);

#ifdef __cplusplus
}
#endif
#endif /* OMC_H */
