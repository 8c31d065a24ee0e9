// omc_api_chain_bounds.hip -- omc_price_american_chain_bounds (include/omc_chain_bounds.h): the
// Andersen-Broadie bounds of n quotes of one expiry with everything that depends on neither the strike nor the side done
// once.  run_bounds' flow (omc_api_bounds.hip) with the entries side by side:
//     fitting paths -> S                                   once
//     per entry: enqueue_lsm on S -> its betas;  lsm_crit_build -> its tables
//     per group of up to chain_bounds_group_max entries:   chain lower sweep (each lower pair once) -> every entry's sums
//     outer paths -> So (Heston: and Vo)                   once
//     per group:  chain inner sweep in run_bounds' launches over blocks of outer paths (each inner pair once per group)
//                 -> every entry's Q^;  per entry: bounds_walk -> its samples and sums;  the group's Q^ and samples out
// The workspace is c->bnd: outer paths | Heston: their variance state | per entry: betas, tables, sums [16], step count | the
// simulated step count | per slot of a group: partials, Q^, samples.  One stream, no host wait before the end.
#include <algorithm>

#include "../../include/omc_chain_bounds.h"
#include "omc_chain_bounds.h"
#include "omc_ctx.h"
#include "omc_heston_bounds.h"

using namespace omc::abi;

static_assert(OMC_CHAIN_BOUNDS_MAX == omc::kChainBoundsMax, "the header states the kernels' cap");

namespace {
constexpr double kMaxItemPairs = 4294967296.0;     // run_bounds' limits, per entry
constexpr double kMaxInnerSteps = 549755813888.0;
constexpr double kLaunchSteps = 1073741824.0;      // 2^30 / d worst-case inner path steps per launch: a pair never runs past N
}  // namespace

extern "C" int omc_price_american_chain_bounds(omc_ctx* c, const omc_params* p, const omc_chain_entry* e, int n,
                                               const omc_bounds_config* cfg, const double* betas, double* betas_out,
                                               double* q_out, double* samples_out, omc_bounds* out,
                                               omc_chain_bounds_info* info)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!p || !e || !cfg || !out) return fail(-7, "null params, entries, bounds config or result pointer.");
    if (n < 1 || n > OMC_CHAIN_MAX) return fail(-42, "a chain of price bounds has 1 .. 256 entries.");
    for (int i = 0; i < n; ++i) {
        if (!(std::isfinite(e[i].K) && e[i].K > 0.0)) return fail(-4, "an entry's strike must be finite and positive.");
        if (e[i].is_put != 0 && e[i].is_put != 1) return fail(-4, "an entry's is_put must be 0 or 1.");
    }
    omc_params q0 = *p;  // (p->K and p->is_put are ignored)
    q0.K = e[0].K;
    q0.is_put = e[0].is_put;
    if ((rc = check_params(&q0))) return rc;
    const bool heston = p->model == OMC_MODEL_HESTON;
    if (heston && p->heston_scheme != OMC_HESTON_REFERENCE_CLAMP && p->heston_scheme != OMC_HESTON_FULL_TRUNCATION)
        return fail(-46, "chain price bounds under Heston take the reference or the full-truncation scheme.");
    if (cfg->regressors != 0) return fail(-4, "chain price bounds take a policy on the spot (regressors 0).");
    for (int i = 0; i < n; ++i)
        if (e[i].exercise_every != 0)
            return fail(-44, "chain price bounds are those of the all-dates game: an entry's exercise_every must be 0.");
    if (c->distributed()) return fail(-43, "chain price bounds run on one GPU.");
    if (c->bounds_every >= 2 || c->bounds_cv != 0 || c->bounds_subopt != 0)
        return fail(-45, "chain price bounds take none of the options bounds_exercise_every, bounds_control_variate and "
                         "bounds_suboptimality.");
    const int policy = cfg->policy;
    if (policy != OMC_SEM_REFERENCE && policy != OMC_SEM_TEXTBOOK && policy != OMC_SEM_TWO_PASS && policy != OMC_POLICY_GIVEN)
        return fail(-4, "unknown policy (reference, textbook, two_pass or given).");
    if (policy == OMC_POLICY_GIVEN && !betas) return fail(-7, "policy 'given' needs a betas table per entry.");
    const int64_t nl = cfg->n_lower, no = cfg->n_outer, ni = cfg->n_inner;
    if (nl < 2 || no < 2 || ni < 2 || (nl & 1) || (no & 1) || (ni & 1))
        return fail(-3, "n_lower, n_outer and n_inner must be even and at least 2 (antithetic pairs).");
    const int N = p->n_steps;
    const size_t n1 = (size_t)N + 1;
    const double work1 = (double)ni * 0.5 * (double)N * (double)(N + 1);  // worst-case inner steps of one outer path
    if ((double)no * (double)(N + 1) * (double)ni > kMaxItemPairs || (double)no * work1 > kMaxInnerSteps)
        return fail(-16, "bounds request too large: n_outer (N+1) n_inner must be <= 2^32 and n_outer n_inner N (N+1) / 2 "
                         "<= 2^39.");
    hipStream_t st = c->stream;
    const bool fitted = policy != OMC_POLICY_GIVEN;
    const int64_t M = fitted ? p->n_paths : 2;
    omc::LsmWorkspace w;
    if ((rc = prepare_lsm(c, M, N, p->r, p->T, policy == OMC_SEM_TWO_PASS, true, &w))) return rc;
    const int G = std::min(n, omc::chain_bounds_group_max(N));  // entries per group: the cap, or what the tables' LDS allows
    const int ngroups = (n + G - 1) / G;
    const int d = heston ? 2 : 1;  // normals per step
    // the workspace
    const size_t path_bytes = up256(sizeof(float) * n1 * (size_t)no);
    const size_t o_vo = path_bytes;
    const size_t o_betas = o_vo + (heston ? path_bytes : 0);
    const size_t betas_bytes = sizeof(double) * 4 * n1, tab_bytes = up256(sizeof(uint32_t) * 8 * n1);
    const size_t o_tab = o_betas + up256(betas_bytes * (size_t)n);
    const size_t o_res = o_tab + tab_bytes * (size_t)n;
    const size_t o_steps = o_res + up256(sizeof(double) * 16 * (size_t)n);
    const size_t o_slot = o_steps + up256(sizeof(unsigned long long) * ((size_t)n + 1));
    const size_t part_bytes = up256(sizeof(double) * 8 * omc::kMaxLsmBlocks);
    const size_t q_bytes = up256(sizeof(double) * (size_t)no * (size_t)N), smp_bytes = up256(sizeof(double) * (size_t)no);
    const size_t slot_bytes = part_bytes + q_bytes + smp_bytes;
    if ((rc = c->bnd.ensure(o_slot + slot_bytes * (size_t)G))) return rc;
    char* b = (char*)c->bnd.p;
    double* dbetas = (double*)(b + o_betas);
    double* dres = (double*)(b + o_res);
    unsigned long long* dsteps = (unsigned long long*)(b + o_steps);  // [n] the entries', then the simulated steps

    omc::BoundsArgs a{};  // the call's common arguments (K, is_put, the policy and the outputs are the entries')
    a.N = N;
    a.s0 = (float)p->S0;  // the generator's start value, so every spot is the generator's
    a.k0 = (uint32_t)p->seed; a.k1 = (uint32_t)(p->seed >> 32);
    a.D = w.D;
    a.n_lower = nl; a.stream_lower = (uint32_t)cfg->stream_lower;
    a.So = (float*)b; a.n_outer = no; a.half_inner = ni / 2; a.stream_inner = (uint32_t)cfg->stream_inner;
    const omc::DiffusionLaw law{heston ? 1 : 0, heston ? p->heston_scheme : 0, p->r, p->sigma, p->T, p->v0, p->kappa,
                                p->theta, p->xi, p->rho, heston ? (const float*)(b + o_vo) : nullptr};
    // group gi's argument block: entry k of the group in slot k
    auto group = [&](int gi) {
        omc::ChainBoundsGroup g{};
        const int i0 = gi * G;
        g.E = std::min(G, n - i0);
        g.steps_sim = dsteps + n;
        for (int k = 0; k < g.E; ++k) {
            const int i = i0 + k;
            char* slot = b + o_slot + slot_bytes * (size_t)k;
            omc::ChainBoundsEntry& x = g.e[k];
            x.K = e[i].K; x.invK = 1.0 / e[i].K; x.is_put = e[i].is_put;
            x.betas = dbetas + 4 * n1 * (size_t)i;
            x.tab = (const uint32_t*)(b + o_tab + tab_bytes * (size_t)i);
            x.part = (double*)slot; x.q = (double*)(slot + part_bytes); x.samples = (double*)(slot + part_bytes + q_bytes);
            x.steps = dsteps + i;
        }
        return g;
    };

    HIP_TRY(hipEventRecord(c->ev[0], st));
    // ---- the policies
    if (fitted) {  // omc_lsm_poly's fits of every entry on the ONE matrix of fitting paths
        float* S = nullptr;
        int64_t ld = 0;
        if ((rc = ensure_paths(c, &q0, Storage::full_only, &S, &ld))) return rc;
        if ((rc = enqueue_paths(c, &q0, S, ld, false))) return rc;
        for (int i = 0; i < n; ++i) {
            if (i) {  // the workspace as prepare_lsm hands it to a single call
                HIP_TRY(hipMemsetAsync(w.gmom, 0, sizeof(double) * 8 * n1, st));
                HIP_TRY(hipMemsetAsync(w.betas, 0, betas_bytes, st));
            }
            omc::LsmProblem prob{S, ld, M, N, e[i].is_put, e[i].K, p->r, p->T};
            if ((rc = enqueue_lsm(c, prob, w, policy, false))) return rc;
            HIP_TRY(hipMemcpyAsync(dbetas + 4 * n1 * (size_t)i, w.betas, betas_bytes, hipMemcpyDeviceToDevice, st));
        }
    } else {  // `betas` is caller memory
        HIP_TRY(hipMemcpyAsync(dbetas, betas, betas_bytes * (size_t)n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    HIP_TRY(hipEventRecord(c->ev[1], st));
    for (int i = 0; i < n; ++i) {  // the stored-path tables of every policy
        omc::CritArgs ct;
        ct.betas = dbetas + 4 * n1 * (size_t)i; ct.tab = (uint32_t*)(b + o_tab + tab_bytes * (size_t)i);
        ct.N = N; ct.is_put = e[i].is_put; ct.K = e[i].K; ct.irr_every = c->pass2_irr_every;
        HIP_TRY(omc::lsm_crit_build(st, ct));
    }
    // ---- the lower bounds
    for (int gi = 0; gi < ngroups; ++gi) {
        const omc::ChainBoundsGroup g = group(gi);
        double* res[omc::kChainBoundsMax] = {};
        for (int k = 0; k < g.E; ++k) res[k] = dres + 16 * (size_t)(gi * G + k);
        HIP_TRY(omc::chain_bounds_lower(st, a, law, g, res));
    }
    HIP_TRY(hipEventRecord(c->ev[2], st));
    // ---- the upper bounds
    if (heston)
        HIP_TRY(omc::launch_heston_paths_sv(st, path_spec(c, p, p->r, (float*)a.So, no, no, cfg->stream_outer, 0), (float*)law.Vo));
    else
        HIP_TRY(omc::launch_gbm_paths(st, (float*)a.So, no, no, N, p->S0, p->r, p->sigma, p->T, p->seed,
                                      (uint32_t)cfg->stream_outer, 0, 1, c->gbm_vec));
    HIP_TRY(hipMemsetAsync(dsteps, 0, sizeof(unsigned long long) * ((size_t)n + 1), st));
    // launches over blocks of outer paths, each at most kLaunchSteps / d inner path steps even if no policy ever exercises
    int64_t blk = (int64_t)(kLaunchSteps / (double)d / work1);
    blk = blk < 1 ? 1 : (blk > no ? no : blk);
    for (int gi = 0; gi < ngroups; ++gi) {
        const omc::ChainBoundsGroup g = group(gi);
        for (int64_t i0 = 0; i0 < no; i0 += blk)
            HIP_TRY(omc::chain_bounds_inner(st, a, law, g, i0, no - i0 < blk ? no - i0 : blk));
        for (int k = 0; k < g.E; ++k) {  // the walk is the single call's, on the entry's own buffers
            const size_t i = (size_t)(gi * G + k);
            HIP_TRY(omc::bounds_walk(st, omc::chain_bounds_entry_args(a, g.e[k]), dres + 16 * i + 8));
            // (the next group reuses the slot: stream order keeps the copies in front of its sweeps)
            if (q_out)
                HIP_TRY(hipMemcpyAsync(q_out + (size_t)no * (size_t)N * i, g.e[k].q, sizeof(double) * (size_t)no * (size_t)N,
                                       hipMemcpyDeviceToHost, st));
            if (samples_out)
                HIP_TRY(hipMemcpyAsync(samples_out + (size_t)no * i, g.e[k].samples, sizeof(double) * (size_t)no,
                                       hipMemcpyDeviceToHost, st));
        }
    }
    HIP_TRY(hipEventRecord(c->ev[3], st));
    std::vector<double> h(16 * (size_t)n);
    std::vector<unsigned long long> steps((size_t)n + 1);
    HIP_TRY(hipMemcpyAsync(h.data(), dres, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(steps.data(), dsteps, sizeof(unsigned long long) * steps.size(), hipMemcpyDeviceToHost, st));
    if (betas_out) HIP_TRY(hipMemcpyAsync(betas_out, dbetas, betas_bytes * (size_t)n, hipMemcpyDeviceToHost, st));
    if ((rc = wait_stream(c))) return rc;
    omc_chain_bounds_info inf;
    memset(&inf, 0, sizeof inf);
    inf.inner_path_steps_simulated = (int64_t)steps[(size_t)n];
    inf.n_groups = ngroups;
    inf.entries_per_group = omc::chain_bounds_group_max(N);
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    inf.ms_fit = ms;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[1], c->ev[2]));
    inf.ms_lower = ms;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
    inf.ms_upper = ms;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[3]));
    inf.ms_total = ms;
    for (int i = 0; i < n; ++i) {  // as run_bounds fills a single call's result
        const double* hi = h.data() + 16 * (size_t)i;
        omc_bounds& o = out[i];
        memset(&o, 0, sizeof o);
        mean_and_se(hi[0], hi[1], (double)(nl / 2), &o.lower, &o.se_lower);  // pair means are the samples
        mean_and_se(hi[8], hi[9], (double)(no / 2), &o.upper, &o.se_upper);
        o.ci_lo = o.lower - 1.96 * o.se_lower;
        o.ci_hi = o.upper + 1.96 * o.se_upper;
        o.n_lower = nl; o.n_outer = no; o.n_inner = ni;
        o.n_exercised_lower = (int64_t)llround(hi[2]);
        o.inner_path_steps = (int64_t)steps[(size_t)i];
        o.ms_fit = inf.ms_fit; o.ms_lower = inf.ms_lower; o.ms_upper = inf.ms_upper; o.ms_total = inf.ms_total;
    }
    if (info) *info = inf;
    return 0;
}
