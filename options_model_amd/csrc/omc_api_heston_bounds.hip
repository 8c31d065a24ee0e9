// omc_api_heston_bounds.hip -- Andersen-Broadie price bounds of American options under the Heston model and the Heston
// generator that keeps the variance state (include/omc.h): omc_price_american_bounds' flow
// (run_bounds, omc_api_bounds.hip) with the Heston generator writing the matrices and the kernels of omc_heston_bounds.hip
// simulating the fresh paths from the outer (spot, variance) state.  With cfg->regressors = OMC_HESTON_REG_SPOT_VARIANCE
// (section 21) the policy is the flow's own -- a table [N+1][8] on the spot and the variance state, fitted by
// omc_heston_sv_bounds.hip on the generator's kept (S, V) matrices, or the caller's -- with that file's sweeps and walk.
#include "omc_ctx.h"
#include "omc_heston_bounds.h"
#include "omc_heston_sv_bounds.h"

using namespace omc::abi;

extern "C" int omc_heston_paths_sv_f32(omc_ctx* c, float* S, float* V, int64_t ld, int64_t n_paths, int n_steps, double S0,
                                       double r, double T, double v0, double kappa, double theta, double xi, double rho,
                                       uint64_t seed, uint64_t stream, uint64_t pair_offset, int scheme)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if (!(S0 > 0) || !(T > 0)) return fail(-1, "S0, K, T must be positive.");
    // (full truncation stores negative variance states, and a stored state is a start state: the float comparison lets NaN fail)
    if (!(rho >= -1.0 && rho <= 1.0) || !(v0 >= 0 || (scheme == 1 && v0 < 0))) return fail(-5, "invalid Heston parameters.");
    if ((rc = check_sizes(n_paths, n_steps))) return rc;
    if ((rc = check_matrix(S, ld, n_paths))) return rc;
    if (!V) return fail(-7, "null variance matrix pointer.");
    if (n_paths & 1) return fail(-3, "antithetic layout needs an even n_paths.");
    if ((rc = check_heston_scheme(scheme, kappa, theta, xi))) return rc;
    omc::PathSpec s{};
    s.model = 1; s.scheme = scheme; s.n_paths = n_paths; s.n_steps = n_steps; s.S0 = S0; s.r = r; s.T = T;
    s.v0 = v0; s.kappa = kappa; s.theta = theta; s.xi = xi; s.rho = rho;
    s.seed = seed; s.pair_offset = pair_offset; s.stream = (uint32_t)stream; s.S = S; s.ld = ld;
    HIP_TRY(omc::launch_heston_paths_sv(c->stream, s, V));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// omc_price_american_bounds_heston with the policy on the spot and the variance state (p and cfg checked by the caller up to
// the selector)
static int heston_sv_bounds(omc_ctx* c, const omc_params* p, const omc_bounds_config* cfg, const double* betas,
                            double* betas_out, double* q_out, double* samples_out, omc_bounds* out)
{
    if (cfg->policy == OMC_SEM_REFERENCE || cfg->policy == OMC_SEM_TWO_PASS)
        return fail(-4, "the spot + variance policy is fitted by textbook Longstaff-Schwartz (policy textbook) or given.");
    const double vbar = p->v0 > p->theta ? p->v0 : p->theta;  // a scale for conditioning only
    if (!(vbar > 0)) return fail(-5, "the spot + variance policy scales the variance by max(v0, theta), which must be positive.");
    const int N = p->n_steps;
    if (N > omc::kHestonSvMaxSteps) return fail(-16, "the spot + variance policy takes at most 512 dates.");
    omc::BoundsArgs a{};
    omc::HestonSvLaw l{{1, p->heston_scheme, p->r, p->sigma, p->T, p->v0, p->kappa, p->theta, p->xi, p->rho, nullptr}, nullptr,
                       1.0 / vbar};
    const bool fitted = cfg->policy != OMC_POLICY_GIVEN;
    const int64_t ld_fit = padded_ld(p->n_paths);  // ensure_paths' leading dimension of the fitting paths
    const size_t pol_bytes = sizeof(double) * omc::kRunnerupCols * (size_t)(N + 1);
    // the flow's room: outer variance state | variance state of the fitting paths | the policy | the fit's partial sums
    size_t o_fit = 0, o_pol = 0, o_part = 0;
    BoundsFlow f;
    f.d = 2;  // two normals per step
    if (cfg->n_outer > 0) {  // (sizes are checked in run_bounds, before the room is used)
        o_fit = up256(sizeof(float) * (size_t)(N + 1) * (size_t)cfg->n_outer);
        o_pol = o_fit + (fitted ? up256(sizeof(float) * (size_t)(N + 1) * (size_t)ld_fit) : 0);
        o_part = o_pol + up256(pol_bytes);
        f.extra_bytes = o_part + sizeof(double) * omc::kRunnerupSlots * omc::kRunnerupFitBlocks;
    }
    char* room = nullptr;
    f.bind = [&](const omc::BoundsArgs& common, char* extra) {
        a = common;
        a.s0 = (float)p->S0;  // the generator's start value, so every spot is the generator's
        l.h.Vo = (const float*)extra;
        l.pol = (const double*)(extra + o_pol);
        room = extra;
    };
    f.own_policy = [&](const omc::LsmWorkspace& w, float* S, int64_t ld) -> int {
        double* pol = (double*)(room + o_pol);
        if (!S) {  // the caller's table; `betas` is caller memory
            HIP_TRY(hipMemcpyAsync(pol, betas, pol_bytes, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            return 0;
        }
        if (ld != ld_fit) return fail(999, "the fitting paths' leading dimension changed under the spot + variance fit.");
        float* V = (float*)(room + o_fit);
        HIP_TRY(omc::launch_heston_paths_sv(c->stream, path_spec(c, p, p->r, S, ld), V));
        omc::HestonSvFit fit{};
        fit.S = S; fit.V = V; fit.ld = ld; fit.M = p->n_paths;
        fit.N = N; fit.is_put = a.is_put; fit.K = a.K; fit.invK = a.invK; fit.inv_vbar = l.inv_vbar;
        fit.D = w.D; fit.x_ex = w.sx; fit.tex = w.tex;
        fit.part = (double*)(room + o_part); fit.pol = pol;
        HIP_TRY(omc::heston_sv_fit(c->stream, fit));
        return 0;
    };
    f.lower = [&](hipStream_t st, double* res) { return omc::heston_sv_lower(st, a, l, res); };
    f.outer = [&](hipStream_t st) {  // the outer paths: spots and variance state, KEEP
        return omc::launch_heston_paths_sv(st, path_spec(c, p, p->r, (float*)a.So, a.n_outer, a.n_outer, cfg->stream_outer, 0),
                                           (float*)l.h.Vo);
    };
    f.inner = [&](hipStream_t st, int64_t i0, int64_t ni) { return omc::heston_sv_inner(st, a, l, i0, ni); };
    f.walk = [&](hipStream_t st, double* res) { return omc::heston_sv_walk(st, a, l, res); };
    f.read_policy = [&](hipStream_t st, double* host) {
        return hipMemcpyAsync(host, l.pol, pol_bytes, hipMemcpyDeviceToHost, st);
    };
    return run_bounds(c, p, cfg, betas, betas_out, q_out, samples_out, out, f);
}

extern "C" int omc_price_american_bounds_heston(omc_ctx* c, const omc_params* p, const omc_bounds_config* cfg,
                                                const double* betas, double* betas_out, double* q_out,
                                                double* samples_out, omc_bounds* out)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!cfg || !out) return fail(-7, "null bounds config or result pointer.");
    if ((rc = check_params(p))) return rc;
    if (p->model != OMC_MODEL_HESTON) return fail(-12, "these price bounds are for the Heston model (GBM: omc_price_american_bounds).");
    if (p->heston_scheme != OMC_HESTON_REFERENCE_CLAMP && p->heston_scheme != OMC_HESTON_FULL_TRUNCATION)
        return fail(-12, "price bounds under Heston take the reference or the full-truncation scheme, not the calibrator's or QE.");
    if (cfg->regressors == OMC_HESTON_REG_SPOT_VARIANCE)
        return heston_sv_bounds(c, p, cfg, betas, betas_out, q_out, samples_out, out);
    if (cfg->regressors != OMC_HESTON_REG_SPOT) return fail(-4, "unknown regressors (spot or spot + variance).");
    omc::BoundsArgs a{};
    omc::DiffusionLaw h{1, p->heston_scheme, p->r, p->sigma, p->T, p->v0, p->kappa, p->theta, p->xi, p->rho, nullptr};
    BoundsFlow f;
    one_asset_flow(f, a, h, h, p, cfg);
    f.fit_paths = [&](float* S, int64_t ld) { return enqueue_paths(c, p, S, ld, false); };
    f.outer = [&](hipStream_t st) {  // the outer paths: spots and variance state, KEEP
        return omc::launch_heston_paths_sv(st, path_spec(c, p, p->r, (float*)a.So, a.n_outer, a.n_outer, cfg->stream_outer, 0),
                                           (float*)h.Vo);
    };
    return run_bounds(c, p, cfg, betas, betas_out, q_out, samples_out, out, f);
}
