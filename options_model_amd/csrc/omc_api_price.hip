// omc_api_price.hip -- one problem per call (include/omc.h): path generators, the backward induction on caller matrices,
// the fused pricing, European, the pass-2 tables check, pathwise Greeks, barrier options, the calibrator's inner loop.
#include "omc_ctx.h"
#include "omc_barrier.h"
#include "omc_crit.h"
#include "omc_greeks.h"

using namespace omc::abi;

extern "C" {

// ------------------------------------------------------------------ path generation
int omc_gbm_paths_f32(omc_ctx* c, float* S, int64_t ld, int64_t n_paths, int n_steps, double S0,
                      double r, double sigma, double T, uint64_t seed, uint64_t stream,
                      uint64_t pair_offset, int antithetic)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if (!(S0 > 0) || !(T > 0)) return fail(-1, "S0, K, T must be positive.");
    if (!(sigma > 0)) return fail(-5, "S0, K, T, and sigma must be positive.");
    if ((rc = check_sizes(n_paths, n_steps))) return rc;
    if ((rc = check_matrix(S, ld, n_paths))) return rc;
    if (antithetic && (n_paths & 1)) return fail(-3, "antithetic layout needs an even n_paths.");
    HIP_TRY(omc::launch_gbm_paths(c->stream, S, ld, n_paths, n_steps, S0, r, sigma, T, seed,
                                  (uint32_t)stream, pair_offset, antithetic, c->gbm_vec));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int omc_heston_paths_f32(omc_ctx* c, float* S, int64_t ld, int64_t n_paths, int n_steps, double S0,
                         double r, double T, double v0, double kappa, double theta, double xi,
                         double rho, uint64_t seed, uint64_t stream, uint64_t pair_offset,
                         int scheme)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if (!(S0 > 0) || !(T > 0)) return fail(-1, "S0, K, T must be positive.");
    if (!(rho >= -1.0 && rho <= 1.0) || !(v0 >= 0)) return fail(-5, "invalid Heston parameters.");
    if ((rc = check_sizes(n_paths, n_steps))) return rc;
    if ((rc = check_matrix(S, ld, n_paths))) return rc;
    if (n_paths & 1) return fail(-3, "antithetic layout needs an even n_paths.");
    if ((rc = check_heston_scheme(scheme, kappa, theta, xi))) return rc;
    HIP_TRY(omc::launch_heston_paths(c->stream, S, ld, n_paths, n_steps, S0, r, T, v0, kappa, theta,
                                     xi, rho, seed, (uint32_t)stream, pair_offset, scheme,
                                     c->heston_vec));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int omc_gbm_paths_from_normals_f32(omc_ctx* c, float* S, int64_t ld, int64_t n_paths, int n_steps,
                                   double S0, double r, double sigma, double T, const float* Z,
                                   int64_t ldz, int antithetic)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if (!(S0 > 0) || !(T > 0)) return fail(-1, "S0, K, T must be positive.");
    if ((rc = check_sizes(n_paths, n_steps))) return rc;
    if ((rc = check_matrix(S, ld, n_paths))) return rc;
    if (!Z) return fail(-7, "null normals pointer.");
    if (antithetic && (n_paths & 1)) return fail(-3, "antithetic layout needs an even n_paths.");
    if (ldz < (antithetic ? n_paths / 2 : n_paths)) return fail(-6, "ldz too small.");
    HIP_TRY(omc::launch_gbm_from_normals(c->stream, S, ld, n_paths, n_steps, S0, r, sigma, T, Z, ldz,
                                         antithetic));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int omc_heston_paths_from_normals_f32(omc_ctx* c, float* S, int64_t ld, int64_t n_paths,
                                      int n_steps, double S0, double r, double T, double v0,
                                      double kappa, double theta, double xi, double rho,
                                      const float* Z1, const float* Z2, int64_t ldz, int scheme)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if (!(S0 > 0) || !(T > 0)) return fail(-1, "S0, K, T must be positive.");
    // (a stored variance state is a start state, so schemes 0, 1 and 2 take a negative v0 as it is; QE's moments of the next
    // variance need v0 >= 0: the float comparisons let NaN fail)
    if (!(rho >= -1.0 && rho <= 1.0) || (scheme == 3 && !(v0 >= 0))) return fail(-5, "invalid Heston parameters.");
    if ((rc = check_sizes(n_paths, n_steps))) return rc;
    if ((rc = check_matrix(S, ld, n_paths))) return rc;
    if (!Z1 || !Z2) return fail(-7, "null normals pointer.");
    if (n_paths & 1) return fail(-3, "antithetic layout needs an even n_paths.");
    if (ldz < n_paths / 2) return fail(-6, "ldz too small.");
    if ((rc = check_heston_scheme(scheme, kappa, theta, xi))) return rc;
    HIP_TRY(omc::launch_heston_from_normals(c->stream, S, ld, n_paths, n_steps, S0, r, T, v0, kappa,
                                            theta, xi, rho, Z1, Z2, ldz, scheme));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int omc_philox4x32_10(omc_ctx* c, const uint32_t* in, uint32_t* out, int n)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if (!in || !out || n <= 0) return fail(-7, "bad arguments.");
    if ((rc = c->scratch.ensure(sizeof(uint32_t) * 10 * (size_t)n))) return rc;
    uint32_t* din = (uint32_t*)c->scratch.p;
    uint32_t* dout = din + 6 * (size_t)n;
    HIP_TRY(hipMemcpyAsync(din, in, sizeof(uint32_t) * 6 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(omc::launch_philox_kat(c->stream, din, dout, n));
    HIP_TRY(hipMemcpyAsync(out, dout, sizeof(uint32_t) * 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int omc_gbm_normals_f32(omc_ctx* c, float* Z, int64_t ldz, int64_t n_pairs, int n_steps,
                        uint64_t seed, uint64_t stream, uint64_t pair_offset)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if (!Z || n_pairs <= 0 || n_steps <= 0 || ldz < n_pairs) return fail(-7, "bad arguments.");
    HIP_TRY(omc::launch_gbm_normals(c->stream, Z, ldz, n_pairs, n_steps, seed, (uint32_t)stream,
                                    pair_offset));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// ------------------------------------------------------------------ backward induction
int omc_lsm_poly(omc_ctx* c, const float* S, int64_t ld, int64_t n_paths, int n_steps, double K,
                 double r, double T, int is_put, int semantics, omc_result* res, double* betas_out,
                 float* sx_out, int32_t* tex_out)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if ((rc = check_lsm_args(S, ld, n_paths, n_steps, K, r, T))) return rc;
    if (semantics < 0 || semantics > 2) return fail(-4, "unknown semantics.");
    if (!res) return fail(-7, "null result pointer.");
    omc::LsmWorkspace w;
    if ((rc = prepare_lsm(c, n_paths, n_steps, r, T, semantics == OMC_SEM_TWO_PASS, betas_out != nullptr, &w))) return rc;
    omc::LsmProblem p{S, ld, n_paths, n_steps, is_put ? 1 : 0, K, r, T};
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    if ((rc = enqueue_lsm(c, p, w, semantics, sx_out || tex_out))) return rc;
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    if ((rc = copy_outputs(c, w, n_paths, n_steps, betas_out, sx_out, tex_out))) return rc;
    if ((rc = check_p2p(c, c->hres, 1))) return rc;
    fill_result(res, c->hres, c->distributed() ? n_paths * c->world : n_paths, c->distributed() ? c->world : 1);
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    res->ms_lsm = ms;
    res->ms_total = ms;
    return 0;
}

int omc_lsm_apply_frozen(omc_ctx* c, const float* S, int64_t ld, int64_t n_paths, int n_steps,
                         double K, double r, double T, int is_put, const double* betas,
                         omc_result* res, float* sx_out, int32_t* tex_out)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if ((rc = check_lsm_args(S, ld, n_paths, n_steps, K, r, T))) return rc;
    if (!betas || !res) return fail(-7, "null pointer.");
    omc::LsmWorkspace w;
    if ((rc = prepare_lsm(c, n_paths, n_steps, r, T, false, true, &w))) return rc;
    if ((rc = upload_fits(c, w, betas, n_steps))) return rc;
    omc::LsmProblem p{S, ld, n_paths, n_steps, is_put ? 1 : 0, K, r, T};
    HIP_TRY(omc::lsm_pass2_apply(c->stream, p, w, sx_out || tex_out));
    if ((rc = copy_outputs(c, w, n_paths, n_steps, nullptr, sx_out, tex_out))) return rc;
    fill_result(res, c->hres, n_paths);
    return 0;
}

// The per-step sweep with EXTERNALLY supplied continuation values: cont is a device float32 matrix
// [n_steps+1][ldc]; at step t an in-the-money path that may still exercise does so iff
// payoff > cont[t][j] (strict).  Everything else -- sticky mask or textbook overwrite, discounting,
// valuation time, the returned statistics -- is the code path of omc_lsm_poly's per-step flows.
int omc_lsm_apply_values(omc_ctx* c, const float* S, int64_t ld, int64_t n_paths, int n_steps, double K,
                         double r, double T, int is_put, int semantics, const float* cont, int64_t ldc,
                         omc_result* res, float* sx_out, int32_t* tex_out)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if ((rc = check_lsm_args(S, ld, n_paths, n_steps, K, r, T))) return rc;
    if (semantics != OMC_SEM_REFERENCE && semantics != OMC_SEM_TEXTBOOK)
        return fail(-4, "continuation values drive the per-step flows only (semantics 0 or 1).");
    if (!cont || !res) return fail(-7, "null pointer.");
    if (ldc < n_paths) return fail(-6, "ldc smaller than n_paths.");
    omc::LsmWorkspace w;
    if ((rc = prepare_lsm(c, n_paths, n_steps, r, T, false, true, &w))) return rc;
    w.cont = cont;
    w.ldc = ldc;
    omc::LsmProblem p{S, ld, n_paths, n_steps, is_put ? 1 : 0, K, r, T};
    for (int t = n_steps; t >= 1; --t) HIP_TRY(omc::lsm_step(c->stream, p, w, semantics, t, false));
    HIP_TRY(omc::lsm_final_reduce(c->stream, p, w, semantics == OMC_SEM_TEXTBOOK ? 0 : 1,
                                  semantics == OMC_SEM_REFERENCE, sx_out || tex_out));
    if ((rc = copy_outputs(c, w, n_paths, n_steps, nullptr, sx_out, tex_out))) return rc;
    c->hres[4] = 0.0;  // no regression sets in this mode
    fill_result(res, c->hres, n_paths);
    return 0;
}

// ------------------------------------------------------------------ fused pricing
int omc_price_american(omc_ctx* c, const omc_params* p, omc_result* res, float* S_keep, int64_t ld)
{
    int rc;
    if ((rc = S_keep ? bind_in(c) : bind(c))) return rc;  // only a caller-provided path matrix is borrowed memory
    if ((rc = check_params(p))) return rc;
    if (!res) return fail(-7, "null result pointer.");
    return price_fused(c, p, nullptr, res, S_keep, ld);
}

int omc_pass2_tables_check(omc_ctx* c, int is_put, double K, int n_steps, const double* betas, const double* cK,
                           int irregular_every, int64_t* mismatches, int* irregular)
{
    if (!c || !betas || !cK || !mismatches || !irregular) return fail(-7, "null pointer.");
    if (n_steps < 1 || n_steps > omc::kMaxSteps || !(K > 0.0)) return fail(-4, "invalid n_steps or strike.");
    HIP_TRY(hipSetDevice(c->device));
    const size_t n1 = (size_t)n_steps + 1;
    const size_t o_cK = sizeof(double) * 4 * n1, o_tab = o_cK + sizeof(double) * n1, o_mism = o_tab + sizeof(uint32_t) * 8 * n1,
                 bytes = o_mism + sizeof(unsigned long long) * 2 * n1;
    int rc;
    if ((rc = c->scratch.ensure(bytes))) return rc;
    char* b = (char*)c->scratch.p;
    HIP_TRY(hipMemcpyAsync(b, betas, sizeof(double) * 4 * n1, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b + o_cK, cK, sizeof(double) * n1, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(b + o_mism, 0, sizeof(unsigned long long) * 2 * n1, c->stream));
    HIP_TRY(omc::lsm_crit_check(c->stream, (const double*)b, (const double*)(b + o_cK), (uint32_t*)(b + o_tab), n_steps,
                                is_put ? 1 : 0, K, irregular_every, (unsigned long long*)(b + o_mism)));
    std::vector<uint32_t> tab(8 * n1);
    HIP_TRY(hipMemcpyAsync(tab.data(), b + o_tab, sizeof(uint32_t) * 8 * n1, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(mismatches, b + o_mism, sizeof(int64_t) * 2 * n1, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t t = 0; t < n1; ++t)
        irregular[t] = tab[8 * t] == omc::kCritIrregular || tab[8 * t + 4] == omc::kCritIrregular;
    return 0;
}

// ------------------------------------------------------------------ pathwise Greeks of the two-pass flow
// Paths as omc_price_american stores them (plan_storage), pass 1 and its fits -- or the caller's fits -- then ONE sweep
// that prices the base, S0 (1 + h) and S0 (1 - h) scenarios with the frozen fits and forms every Greek term from the
// chains' (exercise spot, exercise step) pairs (omc_greeks.hip).  It replaces pass 2: the base scenario takes pass 2's
// decisions with pass 2's expressions, so counts are those of omc_price_american and the price differs only in the
// order of its float64 sum.
int omc_price_american_greeks(omc_ctx* c, const omc_params* p, double bump, const double* betas, double* betas_out,
                              omc_greeks* out)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!out) return fail(-7, "null result pointer.");
    if ((rc = check_params(p))) return rc;
    if (p->semantics != OMC_SEM_TWO_PASS) return fail(-4, "Greeks are those of the two-pass flow (semantics 2).");
    if (!(bump > 0.0 && bump <= 0.5)) return fail(-4, "bump must lie in (0, 0.5].");
    if (c->distributed()) return fail(-10, "the Greeks sweep runs on one GPU.");
    const int64_t M = p->n_paths;
    const int N = p->n_steps;
    float* S = nullptr; int64_t ld = 0;
    const double* cK = nullptr;
    if ((rc = ensure_paths(c, p, Storage::planned, &S, &ld, &cK))) return rc;
    omc::LsmWorkspace w;
    if ((rc = prepare_lsm(c, M, N, p->r, p->T, betas == nullptr, betas_out != nullptr, &w))) return rc;
    if (betas && (rc = upload_fits(c, w, betas, N))) return rc;
    omc::GreeksArgs g;
    g.S = S; g.ld = ld; g.cols = cK ? M / 2 : M;
    g.N = N; g.is_put = p->is_put ? 1 : 0; g.gbm = p->model == OMC_MODEL_GBM ? 1 : 0;
    g.K = p->K; g.S0 = p->S0; g.r = p->r; g.sigma = p->sigma; g.T = p->T; g.h = bump;
    g.D = w.D; g.betas = w.betas; g.cK = cK; g.gmom = betas ? nullptr : w.gmom;
    const int64_t nblk = omc::greeks_blocks(g);
    if ((rc = c->gk_part.ensure(sizeof(double) * omc::kGreeksQ * (size_t)nblk))) return rc;
    if ((rc = c->gk_res.ensure(sizeof(double) * omc::kGreeksQ))) return rc;
    g.part = (double*)c->gk_part.p;
    g.result = (double*)c->gk_res.p;
    omc::LsmProblem prob{S, ld, M, N, p->is_put ? 1 : 0, p->K, p->r, p->T};
    prob.fold_cK = cK;
    w.ev_p1_end = c->ev[4];
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    if ((rc = enqueue_paths(c, p, S, ld, cK != nullptr))) return rc;
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    const bool fit = betas == nullptr && N >= 2;
    if (fit) {
        HIP_TRY(omc::lsm_pass1_moments(c->stream, prob, w));
        HIP_TRY(omc::lsm_solve_betas(c->stream, w.gmom, w.betas, N));
    }
    HIP_TRY(omc::lsm_greeks(c->stream, g, c->ev[5], c->ev[6]));
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    double h[omc::kGreeksQ];
    HIP_TRY(hipMemcpyAsync(h, g.result, sizeof h, hipMemcpyDeviceToHost, c->stream));
    if (betas_out) {
        if (betas) memcpy(betas_out, betas, sizeof(double) * 4 * (size_t)(N + 1));
        else HIP_TRY(hipMemcpyAsync(betas_out, w.betas, sizeof(double) * 4 * (size_t)(N + 1), hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = wait_stream(c))) return rc;
    memset(out, 0, sizeof *out);
    fill_result(&out->base, h, M);
    out->base.folded = cK ? 1 : 0;
    const double Md = (double)M;
    mean_and_se(h[8], h[9], Md, &out->delta, &out->se_delta);
    mean_and_se(h[10], h[11], Md, &out->gamma, &out->se_gamma);
    if (g.gbm) {
        mean_and_se(h[12], h[13], Md, &out->vega, &out->se_vega);
        mean_and_se(h[14], h[15], Md, &out->rho, &out->se_rho);
        mean_and_se(h[16], h[17], Md, &out->theta, &out->se_theta);
    } else {  // no map from the stored spot to the variance path's parameters
        out->vega = out->rho = out->theta = NAN;
        out->se_vega = out->se_rho = out->se_theta = NAN;
    }
    out->bump = bump;
    out->price_up = h[5] / Md;
    out->price_down = h[6] / Md;
    out->n_exercised_up = (int64_t)llround(h[18]);
    out->n_exercised_down = (int64_t)llround(h[19]);
    // no pass 2 (ev[5] .. ev[6] is the Greeks sweep), and with the caller's fits no pass 1 either (ev[4] not recorded)
    if ((rc = read_kernel_times(c->ev, nullptr, &out->base))) return rc;
    float ms = 0;
    if (fit) {
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[1], c->ev[4]));
        out->base.ms_pass1 = ms;
    }
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[5], c->ev[6]));
    out->ms_greeks = ms;
    return 0;
}

int omc_price_european(omc_ctx* c, const omc_params* p, omc_result* res)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if ((rc = check_params(p))) return rc;
    if (!res) return fail(-7, "null result pointer.");
    if ((rc = c->part.ensure(sizeof(double) * 2 * 8 * omc::kMaxLsmBlocks))) return rc;
    if ((rc = c->result.ensure(sizeof(double) * 8))) return rc;
    double* part = (double*)c->part.p;
    HIP_TRY(hipMemsetAsync(part, 0, sizeof(double) * 8 * omc::kMaxLsmBlocks, c->stream));
    int nblk = 0;
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    HIP_TRY(omc::launch_terminal(c->stream, part, &nblk, p->model, p->heston_scheme, p->antithetic,
                                 p->n_paths, p->n_steps, p->S0, p->K, p->r, p->sigma, p->T, p->v0,
                                 p->kappa, p->theta, p->xi, p->rho, p->is_put ? 1 : 0, p->seed,
                                 (uint32_t)p->stream, p->pair_offset));
    HIP_TRY(omc::lsm_finalize(c->stream, part, nullptr, (double*)c->result.p, nblk, 0));
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    HIP_TRY(hipMemcpyAsync(c->hres, c->result.p, sizeof(double) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->hres[2] = 0.0;
    c->hres[4] = 0.0;
    fill_result(res, c->hres, p->n_paths);
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    res->ms_paths = ms;
    res->ms_total = ms;
    return 0;
}

// ------------------------------------------------------------------ barrier options
// The barrier generator (omc_barrier.hip) writes the ENCODED matrix -- the real spot where the option is live, the dead
// spot elsewhere -- and reduces the European knock-out / knock-in sums; the American price is then the unchanged two-pass
// flow (enqueue_lsm) on that full-storage matrix.  European only: the generator without a matrix.
int omc_price_barrier(omc_ctx* c, const omc_params* p, const omc_barrier* b, omc_barrier_result* out, float* S_keep,
                      int64_t ld)
{
    int rc;
    if ((rc = S_keep ? bind_in(c) : bind(c))) return rc;
    if ((rc = check_params(p))) return rc;
    if (!b || !out) return fail(-7, "null barrier or result pointer.");
    if (b->kind < OMC_BARRIER_DOWN_OUT || b->kind > OMC_BARRIER_UP_IN || b->monitoring < OMC_MONITOR_DISCRETE ||
        b->monitoring > OMC_MONITOR_CONTINUOUS || (b->american != 0 && b->american != 1))
        return fail(-15, "unknown barrier kind, monitoring or style.");
    if (!p->antithetic) return fail(-15, "barrier paths are antithetic pairs (antithetic = 1).");
    if (b->american && p->semantics != OMC_SEM_TWO_PASS)
        return fail(-11, "American barrier options are priced by the two-pass flow (semantics 2).");
    if (b->monitoring == OMC_MONITOR_CONTINUOUS && p->model != OMC_MODEL_GBM)
        return fail(-12, "continuous barrier monitoring is available for GBM only.");
    if (!(std::isfinite(b->H) && b->H > 0.0)) return fail(-13, "barrier H must be finite and positive.");
    const int up = (b->kind == OMC_BARRIER_UP_OUT || b->kind == OMC_BARRIER_UP_IN) ? 1 : 0;
    const float thr = omc::barrier_threshold(b->H, up);
    const float s0f = (float)p->S0;
    if (up ? (p->S0 >= b->H || s0f >= thr) : (p->S0 <= b->H || s0f <= thr))
        return fail(-14, "S0 lies on or beyond the barrier (the option is already knocked).");
    if (c->distributed()) return fail(-10, "barrier pricing runs on one GPU.");
    if (S_keep && ld < p->n_paths) return fail(-6, "leading dimension smaller than n_paths.");
    const int64_t M = p->n_paths;
    float* S = S_keep;
    if (b->american && !S && (rc = ensure_paths(c, p, Storage::full_only, &S, &ld))) return rc;
    omc::BarrierGen g{};
    g.paths = path_spec(c, p, p->r, S, S ? ld : 0);
    g.is_put = p->is_put ? 1 : 0; g.up = up;
    g.knock_in = (b->kind == OMC_BARRIER_DOWN_IN || b->kind == OMC_BARRIER_UP_IN) ? 1 : 0;
    g.continuous = b->monitoring == OMC_MONITOR_CONTINUOUS ? 1 : 0;
    g.K = p->K; g.H = b->H;
    const int64_t nblk = omc::barrier_blocks(g);
    if ((rc = c->bar_part.ensure(sizeof(double) * omc::kBarrierQ * (size_t)nblk))) return rc;
    if ((rc = c->bar_res.ensure(sizeof(double) * omc::kBarrierQ))) return rc;
    g.part = (double*)c->bar_part.p;
    g.result = (double*)c->bar_res.p;
    const auto gen = [&](hipStream_t st) { return omc::launch_barrier_paths(st, g); };
    if (b->american) {
        if ((rc = enqueue_generated(c, p, S, ld, gen))) return rc;
    } else {
        HIP_TRY(hipEventRecord(c->ev[0], c->stream));
        HIP_TRY(gen(c->stream));
        HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    }
    double h[omc::kBarrierQ];
    HIP_TRY(hipMemcpyAsync(h, g.result, sizeof h, hipMemcpyDeviceToHost, c->stream));
    omc_result american;
    if ((rc = b->american ? finish_generated(c, p, &american) : wait_stream(c))) return rc;
    memset(out, 0, sizeof *out);
    const double Md = (double)M;
    mean_and_se(h[0], h[1], Md, &out->euro_out, &out->euro_out_se);
    mean_and_se(h[2], h[3], Md, &out->euro_in, &out->euro_in_se);
    out->hit_prob = h[4] / Md;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    out->ms_barrier_paths = ms;
    if (b->american) {
        out->base = american;
    } else {  // the European option of `kind`
        const int q = g.knock_in ? 2 : 0;
        const double e[8] = {h[q], h[q + 1], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        fill_result(&out->base, e, M);
        out->base.n_zero = 0;
        out->base.zero_prob = 0.0;
        out->base.ms_paths = ms;
        out->base.ms_total = ms;
    }
    return 0;
}

// ------------------------------------------------------------------ calibrator inner loop
int omc_heston_price_strikes(omc_ctx* c, int64_t n_paths, int n_steps, double S0, double r, double T,
                             double v0, double kappa, double theta, double xi, double rho,
                             uint64_t seed, uint64_t stream, int scheme, const double* strikes,
                             int n_strikes, int is_put, double* prices, double* stderrs)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if (!(S0 > 0) || !(T > 0)) return fail(-1, "S0, K, T must be positive.");
    if ((rc = check_sizes(n_paths, n_steps))) return rc;
    if (n_paths & 1) return fail(-3, "antithetic layout needs an even n_paths.");
    if ((rc = check_heston_scheme(scheme, kappa, theta, xi))) return rc;
    if (!(rho >= -1.0 && rho <= 1.0) || !(v0 >= 0)) return fail(-5, "invalid Heston parameters.");
    if (!strikes || !prices || n_strikes <= 0) return fail(-7, "bad strike arguments.");
    if (n_paths > (int64_t)65535 * 4096) return fail(-3, "at most 268,431,360 paths per expiry.");
    const size_t st_bytes = sizeof(float) * (size_t)n_paths;
    const size_t k_bytes = sizeof(double) * (size_t)n_strikes;
    if ((rc = c->scratch.ensure(st_bytes + 256 + 3 * k_bytes + omc::payoff_partial_bytes(n_paths, n_strikes)))) return rc;
    float* ST = (float*)c->scratch.p;
    double* Kd = (double*)((char*)c->scratch.p + up256(st_bytes));
    double* out = Kd + n_strikes;
    double* part = out + 2 * (size_t)n_strikes;
    HIP_TRY(hipMemcpyAsync(Kd, strikes, k_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(omc::launch_heston_terminal_store(c->stream, ST, n_paths, n_steps, S0, r, T, v0, kappa, theta,
                                              xi, rho, seed, (uint32_t)stream, 0, scheme));
    HIP_TRY(omc::launch_payoff_means(c->stream, ST, n_paths, Kd, n_strikes, is_put ? 1 : 0, part, out));
    std::vector<double> h(2 * (size_t)n_strikes);
    HIP_TRY(hipMemcpyAsync(h.data(), out, 2 * k_bytes, hipMemcpyDeviceToHost, c->stream));
    if ((rc = wait_stream(c))) return rc;  // (polling: the call lasts ~0.1 ms)
    const double df = std::exp(-r * T), M = (double)n_paths;
    for (int k = 0; k < n_strikes; ++k) {
        double mean, se;
        mean_and_se(h[2 * (size_t)k], h[2 * (size_t)k + 1], M, &mean, &se);
        prices[k] = df * mean;
        if (stderrs) stderrs[k] = df * se;
    }
    return 0;
}

// A whole quote surface in one launch set: what one evaluation of the calibrator's objective asks for
// (heston_calibration.py:283-312, 404-472: ~60 quotes over a handful of expiries, per optimizer iteration).  Every
// expiry is simulated on its own Philox sub-stream (streams[e]) and every quote averaged over ITS expiry's terminal
// spots -- two launches, one table upload, one read-back, one wait, instead of that per expiry; each quote comes back
// with the bits of its own omc_heston_price_strikes(T = expiries[expiry_of[q]], stream = streams[expiry_of[q]]) call.
int omc_heston_price_surface(omc_ctx* c, int64_t n_paths, int n_steps, double S0, double r, double v0, double kappa,
                             double theta, double xi, double rho, uint64_t seed, int scheme, const double* expiries,
                             const uint64_t* streams, int n_expiries, const double* strikes, const int32_t* expiry_of,
                             int n_quotes, int is_put, double* prices, double* stderrs)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if (!(S0 > 0)) return fail(-1, "S0, K, T must be positive.");
    if ((rc = check_sizes(n_paths, n_steps))) return rc;
    if (n_paths & 1) return fail(-3, "antithetic layout needs an even n_paths.");
    if ((rc = check_heston_scheme(scheme, kappa, theta, xi))) return rc;
    if (!(rho >= -1.0 && rho <= 1.0) || !(v0 >= 0)) return fail(-5, "invalid Heston parameters.");
    if (!expiries || !streams || n_expiries <= 0 || n_expiries > 65535) return fail(-7, "bad expiry arguments (1 .. 65535 expiries).");
    if (!strikes || !expiry_of || !prices || n_quotes <= 0) return fail(-7, "bad strike arguments.");
    if (n_paths > (int64_t)65535 * 4096) return fail(-3, "at most 268,431,360 paths per expiry.");
    for (int e = 0; e < n_expiries; ++e)
        if (!(expiries[e] > 0)) return fail(-1, "S0, K, T must be positive.");
    for (int q = 0; q < n_quotes; ++q)
        if (expiry_of[q] < 0 || expiry_of[q] >= n_expiries) return fail(-4, "expiry_of[q] must index the expiries.");
    const int64_t ldst = padded_ld(n_paths);
    const size_t st_bytes = up256(sizeof(float) * (size_t)ldst * (size_t)n_expiries);
    // ONE upload per call: [expiry table | strikes | quote -> expiry] as one host image behind the terminal spots
    const size_t tab_bytes = up256(omc::heston_surface_table_bytes(n_expiries));
    const size_t k_bytes = sizeof(double) * (size_t)n_quotes, e_bytes = up256(sizeof(int32_t) * (size_t)n_quotes);
    const size_t img_bytes = tab_bytes + up256(k_bytes) + e_bytes;
    if ((rc = c->scratch.ensure(st_bytes + img_bytes + 2 * k_bytes + 256 + omc::payoff_partial_bytes(n_paths, n_quotes)))) return rc;
    char* base = (char*)c->scratch.p;
    float* ST = (float*)base;
    char* img_d = base + st_bytes;
    const void* tab = img_d;
    const double* Kd = (const double*)(img_d + tab_bytes);
    const int32_t* eo = (const int32_t*)(img_d + tab_bytes + up256(k_bytes));
    double* out = (double*)(img_d + img_bytes);
    double* part = out + 2 * (size_t)n_quotes;
    // the host image must outlive the asynchronous copy (pageable memory): the context keeps it until the wait below
    c->h_table.resize(img_bytes + sizeof(uint32_t) * (size_t)n_expiries);
    char* img_h = c->h_table.data();
    uint32_t* st32 = (uint32_t*)(img_h + img_bytes);
    for (int e = 0; e < n_expiries; ++e) st32[e] = (uint32_t)streams[e];
    omc::heston_surface_fill_table(img_h, n_steps, r, expiries, st32, n_expiries, kappa, theta, xi, rho);
    memcpy(img_h + tab_bytes, strikes, k_bytes);
    memcpy(img_h + tab_bytes + up256(k_bytes), expiry_of, sizeof(int32_t) * (size_t)n_quotes);
    HIP_TRY(hipMemcpyAsync(img_d, img_h, img_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(omc::launch_heston_terminal_surface(c->stream, ST, ldst, n_paths, n_steps, S0, n_expiries, v0, seed, 0, scheme, tab));
    HIP_TRY(omc::launch_payoff_means_surface(c->stream, ST, ldst, n_paths, Kd, eo, n_quotes, is_put ? 1 : 0, part, out));
    std::vector<double> h(2 * (size_t)n_quotes);
    HIP_TRY(hipMemcpyAsync(h.data(), out, 2 * k_bytes, hipMemcpyDeviceToHost, c->stream));
    if ((rc = wait_stream(c))) return rc;  // (polling: the call lasts ~0.1 ms)
    const double M = (double)n_paths;
    for (int q = 0; q < n_quotes; ++q) {
        const double df = std::exp(-r * expiries[expiry_of[q]]);
        double mean, se;
        mean_and_se(h[2 * (size_t)q], h[2 * (size_t)q + 1], M, &mean, &se);
        prices[q] = df * mean;
        if (stderrs) stderrs[q] = df * se;
    }
    return 0;
}

}  // extern "C"
