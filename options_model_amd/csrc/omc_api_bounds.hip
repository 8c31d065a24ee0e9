// omc_api_bounds.hip -- Andersen-Broadie price bounds of American options (include/omc.h): the policy
// fit, the lower-bound sweep, the outer paths, the inner simulations in launches over blocks of outer paths, the walk.
// run_bounds is that flow, shared with the multi-asset entry point (omc_api_basket_bounds.hip, section 17).
#include "omc_bounds.h"
#include "omc_ctx.h"

using namespace omc::abi;

namespace {
constexpr double kMaxItemPairs = 4294967296.0;   // n_outer (N+1) n_inner
constexpr double kMaxInnerSteps = 549755813888.0;  // 2^39: n_outer n_inner N (N+1) / 2, a never-exercising policy's steps
constexpr double kLaunchSteps = 1073741824.0;    // 2^30 / d worst-case inner path steps per launch of the inner kernel
}  // namespace

namespace omc::abi {

int run_bounds(omc_ctx* c, const omc_params* p, const omc_bounds_config* cfg, const double* betas, double* betas_out,
               double* q_out, double* samples_out, omc_bounds* out, const BoundsFlow& f)
{
    int rc;
    if (c->distributed()) return fail(-10, "price bounds run on one GPU.");
    const int policy = cfg->policy;
    if (policy != OMC_SEM_REFERENCE && policy != OMC_SEM_TEXTBOOK && policy != OMC_SEM_TWO_PASS && policy != OMC_POLICY_GIVEN)
        return fail(-4, "unknown policy (reference, textbook, two_pass or given).");
    if (policy == OMC_POLICY_GIVEN && !betas) return fail(-7, "policy 'given' needs a betas table.");
    const int64_t nl = cfg->n_lower, no = cfg->n_outer, ni = cfg->n_inner;
    if (nl < 2 || no < 2 || ni < 2 || (nl & 1) || (no & 1) || (ni & 1))
        return fail(-3, "n_lower, n_outer and n_inner must be even and at least 2 (antithetic pairs).");
    const int N = p->n_steps;
    const double work1 = (double)ni * 0.5 * (double)N * (double)(N + 1);  // worst-case inner steps of one outer path
    if ((double)no * (double)(N + 1) * (double)ni > kMaxItemPairs || (double)no * work1 > kMaxInnerSteps)
        return fail(-16, "bounds request too large: n_outer (N+1) n_inner must be <= 2^32 and n_outer n_inner N (N+1) / 2 "
                         "<= 2^39.");
    // an exercise schedule (option "bounds_exercise_every" = k >= 2): the flows that bring the scheduled inner sweep take it
    if (c->bounds_every >= 2 && !f.inner_sched)
        return fail(-38, "option bounds_exercise_every: these bounds take no exercise schedule (one asset, a policy on the "
                         "spot: omc_price_american_bounds, omc_price_american_bounds_heston with regressors spot).");
    // the control variate (option "bounds_control_variate" = 1): the flows that bring the controlled sweeps take it
    const bool cv = c->bounds_cv != 0;
    if (cv && !(f.lower_cv && f.inner_cv && (c->bounds_every < 2 || f.inner_sched_cv)))
        return fail(-39, "option bounds_control_variate: these bounds have no control variate (one GBM asset: "
                         "omc_price_american_bounds).");
    // sub-optimality checking (option "bounds_suboptimality" = m >= 1): the all-dates game of the flows that run the shared
    // sweeps and walk; the European check needs the flow's table of E
    const int chk = c->bounds_subopt;
    if (chk >= 1 && (c->bounds_every >= 2 || f.own_policy || !f.inner_check || (cv && !f.inner_check_cv) ||
                     (chk == 2 && !f.euro_table)))
        return fail(-40, "option bounds_suboptimality: these bounds take no sub-optimality check (the all-dates game with a "
                         "policy on the spot or the index; the European check: omc_price_american_bounds).");
    const bool sched = c->bounds_every >= 2;
    // the list-driven sweep: the sub-optimality check's, or that of a flow that takes items out itself (mode 0)
    const bool lst = chk >= 1 || (f.mark_items && f.inner_check && !sched && !cv);
    const omc::BoundsSched sc = sched ? omc::bounds_schedule(N, c->bounds_every) : omc::BoundsSched{};
    hipStream_t st = c->stream;
    const bool fitted = policy != OMC_POLICY_GIVEN;
    const int64_t M = fitted ? p->n_paths : 2;
    omc::LsmWorkspace w;
    if ((rc = prepare_lsm(c, M, N, p->r, p->T, policy == OMC_SEM_TWO_PASS, true, &w))) return rc;
    const bool own = (bool)f.own_policy;  // the flow brings its policy, its walk and its read-back
    if (!fitted && !own && (rc = upload_fits(c, w, betas, N))) return rc;
    if (!fitted && sched) HIP_TRY(omc::bounds_sched_policy(st, w.betas, w.betas, N, sc, false));  // zero rows off the schedule
    // the workspace: outer paths [N+1][n_outer] f32 | the flow's own room | Q^ [n_outer][N] | samples [n_outer] | tables
    // [N+1][8] u32 | partials [8][kPStride] | sums [16] | inner step count | with a schedule: the fit's discounts [J+1] | its
    // fits [J+1][4] | with sub-optimality checking: the keep mask [N][n_outer] u8 | the kept items of one inner launch
    // [blk N] u32 | their count | the kept items per (inner launch, date) u32
    const size_t o_extra = up256(sizeof(float) * (size_t)(N + 1) * (size_t)no);
    const size_t o_q = o_extra + up256(f.extra_bytes);
    const size_t o_smp = o_q + up256(sizeof(double) * (size_t)no * (size_t)N);
    const size_t o_tab = o_smp + up256(sizeof(double) * (size_t)no);
    const size_t o_part = o_tab + up256(sizeof(uint32_t) * 8 * (size_t)(N + 1));
    const size_t o_res = o_part + up256(sizeof(double) * 8 * omc::kMaxLsmBlocks);
    const size_t o_steps = o_res + up256(sizeof(double) * 16);
    const size_t o_fD = o_steps + 256;
    const size_t o_fb = o_fD + (sched ? up256(sizeof(double) * (size_t)(sc.J + 1)) : 0);
    // launches over blocks of outer paths, each at most kLaunchSteps / d inner path steps even if the policy never exercises
    int64_t blk = (int64_t)(kLaunchSteps / (double)f.d / work1);
    blk = blk < 1 ? 1 : (blk > no ? no : blk);
    const size_t o_keep = o_fb + (sched ? sizeof(double) * 4 * (size_t)(sc.J + 1) : 0);
    const size_t o_list = o_keep + (lst ? up256((size_t)N * (size_t)no) : 0);
    const size_t o_cnt = o_list + (lst ? up256(sizeof(uint32_t) * (size_t)blk * (size_t)N) : 0);
    const size_t o_pd = o_cnt + (lst ? 256 : 0);
    const size_t pd_bytes = lst ? sizeof(uint32_t) * (size_t)((no + blk - 1) / blk) * (size_t)N : 0;
    if ((rc = c->bnd.ensure(o_pd + pd_bytes))) return rc;
    char* b = (char*)c->bnd.p;
    double* res = (double*)(b + o_res);

    omc::BoundsArgs a{};  // (s0, a, b: the single-asset flow's, set in its bind)
    a.N = N; a.is_put = p->is_put ? 1 : 0; a.K = p->K; a.invK = 1.0 / p->K;
    a.k0 = (uint32_t)p->seed; a.k1 = (uint32_t)(p->seed >> 32);
    a.D = w.D; a.betas = w.betas; a.tab = (uint32_t*)(b + o_tab);
    a.n_lower = nl; a.stream_lower = (uint32_t)cfg->stream_lower;
    a.So = (float*)b; a.n_outer = no; a.half_inner = ni / 2; a.stream_inner = (uint32_t)cfg->stream_inner;
    a.q = (double*)(b + o_q); a.samples = (double*)(b + o_smp);
    a.steps = (unsigned long long*)(b + o_steps);
    a.part = (double*)(b + o_part);
    f.bind(a, b + o_extra);
    const omc::BoundsCheck ck{chk, (unsigned char*)(b + o_keep), (uint32_t*)(b + o_list), (uint32_t*)(b + o_cnt),
                              (uint32_t*)(b + o_pd), blk};
    // With a schedule the fit is omc_lsm_poly's on the J scheduled dates: its horizon T_v = T (J k) / N counts a short first
    // gap as a whole one, and its discount table is ensure_discounts' for (J, r, T_v)
    omc::LsmWorkspace wf = w;
    double Tv = p->T;
    if (sched && fitted) {
        const int64_t Jk = (int64_t)sc.J * c->bounds_every;
        if (Jk != N) Tv = p->T * (double)Jk / (double)N;
        std::vector<double> hD((size_t)sc.J + 1);
        const double dt = Tv / sc.J;
        for (int k = 0; k <= sc.J; ++k) hD[(size_t)k] = std::exp(-p->r * dt * (double)k);
        wf.D = (double*)(b + o_fD);
        wf.betas = (double*)(b + o_fb);
        HIP_TRY(hipMemcpyAsync(wf.D, hD.data(), sizeof(double) * hD.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));  // hD is pageable host memory
        HIP_TRY(hipMemsetAsync(wf.betas, 0, sizeof(double) * 4 * (size_t)(sc.J + 1), st));
    }

    HIP_TRY(hipEventRecord(c->ev[0], st));
    if (own) {
        float* S = nullptr;
        int64_t ld = 0;
        if (fitted && (rc = ensure_paths(c, p, Storage::full_only, &S, &ld))) return rc;
        if ((rc = f.own_policy(w, S, ld))) return rc;
    } else if (fitted) {  // omc_lsm_poly's fits on the paths of p
        float* S = nullptr;
        int64_t ld = 0;
        if ((rc = ensure_paths(c, p, Storage::full_only, &S, &ld))) return rc;
        if ((rc = f.fit_paths(S, ld))) return rc;
        if (sched) {  // rows 0, tau_1 .. tau_J of the fitting paths, J steps; fit row j is the policy's row tau_j
            HIP_TRY(omc::bounds_sched_gather(st, S, ld, sc));
            omc::LsmProblem prob{S, ld, M, sc.J, a.is_put, p->K, p->r, Tv};
            if ((rc = enqueue_lsm(c, prob, wf, policy, false))) return rc;
            HIP_TRY(omc::bounds_sched_policy(st, wf.betas, w.betas, N, sc, true));
        } else {
            omc::LsmProblem prob{S, ld, M, N, a.is_put, p->K, p->r, p->T};
            if ((rc = enqueue_lsm(c, prob, w, policy, false))) return rc;
        }
    }
    HIP_TRY(hipEventRecord(c->ev[1], st));
    if (!own) {
        omc::CritArgs ct;  // the stored-path tables of the policy
        ct.betas = w.betas; ct.tab = (uint32_t*)a.tab;
        ct.N = N; ct.is_put = a.is_put; ct.K = p->K; ct.irr_every = c->pass2_irr_every;
        HIP_TRY(omc::lsm_crit_build(st, ct));
    }
    HIP_TRY(cv ? f.lower_cv(st, res) : f.lower(st, res));
    HIP_TRY(hipEventRecord(c->ev[2], st));
    HIP_TRY(f.outer(st));
    HIP_TRY(hipMemsetAsync(a.steps, 0, sizeof(unsigned long long), st));
    if (lst) {  // the keep mask of every item; Q^ keeps its shape [n_outer][N], a skipped item's entry reads 0
        const double* cvt = nullptr;
        if (chk == 2) HIP_TRY(f.euro_table(st, &cvt));
        HIP_TRY(hipMemsetAsync(ck.per_date, 0, pd_bytes, st));
        HIP_TRY(chk ? omc::bounds_check_mark(st, a, ck, cvt) : f.mark_items(st, ck));
        HIP_TRY(hipMemsetAsync(a.q, 0, sizeof(double) * (size_t)no * (size_t)N, st));
    }
    if (sched) {  // the scheduled worst case n_inner sum_j (N - tau_j), j = 0 .. J-1
        double launch_work = (double)ni * (double)N;
        for (int j = 1; j < sc.J; ++j) launch_work += (double)ni * (double)(N - (sc.tau1 + (j - 1) * sc.k));
        // Q^ keeps its shape [n_outer][N]; the sweep writes the scheduled columns, the others read 0
        HIP_TRY(hipMemsetAsync(a.q, 0, sizeof(double) * (size_t)no * (size_t)N, st));
        blk = (int64_t)(kLaunchSteps / (double)f.d / launch_work);
        blk = blk < 1 ? 1 : (blk > no ? no : blk);
    }
    for (int64_t i0 = 0; i0 < no; i0 += blk) {
        const int64_t n = no - i0 < blk ? no - i0 : blk;
        if (lst) {  // the block's kept items, then the sweep over them: the count stays on the device
            HIP_TRY(omc::bounds_check_compact(st, a, ck, i0, n));
            HIP_TRY(cv ? f.inner_check_cv(st, ck, i0, n) : f.inner_check(st, ck, i0, n));
        }
        else if (cv) HIP_TRY(sched ? f.inner_sched_cv(st, sc, i0, n) : f.inner_cv(st, i0, n));
        else HIP_TRY(sched ? f.inner_sched(st, sc, i0, n) : f.inner(st, i0, n));
    }
    if (lst) HIP_TRY(omc::bounds_check_walk(st, a, ck, res + 8));
    else if (sched) HIP_TRY(omc::bounds_sched_walk(st, a, sc, res + 8));
    else HIP_TRY(own ? f.walk(st, res + 8) : omc::bounds_walk(st, a, res + 8));
    HIP_TRY(hipEventRecord(c->ev[3], st));
    double h[16];
    unsigned long long steps = 0;
    HIP_TRY(hipMemcpyAsync(h, res, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&steps, a.steps, sizeof steps, hipMemcpyDeviceToHost, st));
    if (betas_out && own) HIP_TRY(f.read_policy(st, betas_out));
    if (betas_out && !own)
        HIP_TRY(hipMemcpyAsync(betas_out, w.betas, sizeof(double) * 4 * (size_t)(N + 1), hipMemcpyDeviceToHost, st));
    if (q_out) HIP_TRY(hipMemcpyAsync(q_out, a.q, sizeof(double) * (size_t)no * (size_t)N, hipMemcpyDeviceToHost, st));
    if (samples_out) HIP_TRY(hipMemcpyAsync(samples_out, a.samples, sizeof(double) * (size_t)no, hipMemcpyDeviceToHost, st));
    if ((rc = wait_stream(c))) return rc;
    memset(out, 0, sizeof *out);
    mean_and_se(h[0], h[1], (double)(nl / 2), &out->lower, &out->se_lower);  // pair means are the samples
    if (cv) out->lower += f.cv_e0;  // the sums are those of the centred pair means
    mean_and_se(h[8], h[9], (double)(no / 2), &out->upper, &out->se_upper);
    out->ci_lo = out->lower - 1.96 * out->se_lower;
    out->ci_hi = out->upper + 1.96 * out->se_upper;
    out->n_lower = nl; out->n_outer = no; out->n_inner = ni;
    out->n_exercised_lower = (int64_t)llround(h[2]);
    out->inner_path_steps = (int64_t)steps;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    out->ms_fit = ms;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[1], c->ev[2]));
    out->ms_lower = ms;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
    out->ms_upper = ms;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[3]));
    out->ms_total = ms;
    return 0;
}

}  // namespace omc::abi

extern "C" int omc_price_american_bounds(omc_ctx* c, const omc_params* p, const omc_bounds_config* cfg,
                                         const double* betas, double* betas_out, double* q_out, double* samples_out,
                                         omc_bounds* out)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!cfg || !out) return fail(-7, "null bounds config or result pointer.");
    if ((rc = check_params(p))) return rc;
    if (p->model != OMC_MODEL_GBM) return fail(-12, "price bounds are available for GBM only.");
    omc::BoundsCvArgs cva{};  // (cva.b == a once bound; read by the controlled sweeps alone)
    omc::BoundsArgs& a = cva.b;
    BoundsFlow f;
    const bool cv = c->bounds_cv != 0;
    const int form = c->bounds_cv_form;
    // the table of E's per-date constants: the control variate's, and the European sub-optimality check's
    if (cv || c->bounds_subopt == 2) f.extra_bytes = sizeof(double) * 4 * ((size_t)p->n_steps + 1);
    f.fit_paths = [&](float* S, int64_t ld) { return enqueue_paths(c, p, S, ld, false); };
    f.bind = [&](const omc::BoundsArgs& common, char* extra) {
        a = common;
        a.s0 = (float)p->S0;  // the generator's start value and step constants, so every spot is the generator's
        omc::gbm_step_constants(p->r, p->sigma, p->T, p->n_steps, &a.a, &a.b);
        cva.r = p->r; cva.sigma = p->sigma; cva.dt = p->T / (double)p->n_steps;
        cva.cv = (double*)extra;
    };
    f.lower = [&](hipStream_t st, double* res) { return omc::bounds_lower(st, a, res); };
    f.outer = [&](hipStream_t st) {
        return omc::launch_gbm_paths(st, (float*)a.So, a.n_outer, a.n_outer, a.N, p->S0, p->r, p->sigma, p->T, p->seed,
                                     (uint32_t)cfg->stream_outer, 0, 1, c->gbm_vec);
    };
    f.inner = [&](hipStream_t st, int64_t i0, int64_t ni) { return omc::bounds_inner(st, a, i0, ni); };
    f.inner_sched = [&](hipStream_t st, const omc::BoundsSched& sc, int64_t i0, int64_t ni) {
        return omc::bounds_sched_inner(st, a, sc, i0, ni);
    };
    // the control variate (option "bounds_control_variate"): the table, then the controlled sweeps
    f.lower_cv = [&](hipStream_t st, double* res) {
        const hipError_t e = omc::bounds_cv_table(st, cva);
        return e != hipSuccess ? e : omc::bounds_lower_cv(st, cva, res);
    };
    f.inner_cv = [&](hipStream_t st, int64_t i0, int64_t ni) { return omc::bounds_inner_cv(st, cva, form, i0, ni); };
    f.inner_sched_cv = [&](hipStream_t st, const omc::BoundsSched& sc, int64_t i0, int64_t ni) {
        return omc::bounds_sched_inner_cv(st, cva, sc, form, i0, ni);
    };
    // sub-optimality checking (option "bounds_suboptimality"): the list-driven sweeps; the European
    // check reads the control variate's table, built here when the control variate has not built it
    f.inner_check = [&](hipStream_t st, const omc::BoundsCheck& k, int64_t i0, int64_t ni) {
        return omc::bounds_check_inner(st, a, k, i0, ni);
    };
    f.inner_check_cv = [&](hipStream_t st, const omc::BoundsCheck& k, int64_t i0, int64_t ni) {
        return omc::bounds_check_inner_cv(st, cva, k, form, i0, ni);
    };
    f.euro_table = [&](hipStream_t st, const double** table) {
        *table = cva.cv;
        return cv ? hipSuccess : omc::bounds_cv_table(st, cva);
    };
    if (cv)  // D[0] = 1; the spot is the generator's float32 start value
        f.cv_e0 = omc::bounds_cv_euro_host((double)(float)p->S0, p->K, p->r, p->sigma,
                                           (double)p->n_steps * (p->T / (double)p->n_steps), p->is_put != 0);
    return run_bounds(c, p, cfg, betas, betas_out, q_out, samples_out, out, f);
}
