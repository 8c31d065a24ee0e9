// omc_api_jump_bounds.hip -- Andersen-Broadie price bounds of American options under jump-diffusion and the jump
// generator as an entry point of its own (include/omc_jump_bounds.h): omc_price_american_bounds' flow
// (run_bounds, omc_api_bounds.hip) with the jump generator (omc_jump.hip; with the variance kept: omc_jump_bounds.hip)
// writing the matrices and the kernels of omc_jump_bounds.hip simulating the fresh paths from the outer spot (Merton) or
// (spot, variance) state (Bates).  lambda = 0 takes the same route: its thresholds are all 2^24, no step jumps, and every
// spot carries the vanilla generator's bits.
#include "omc_ctx.h"
#include "omc_jump_bounds.h"

using namespace omc::abi;

namespace {

// (lambda = 0 leaves the compensator out: 0 * kappa is not formed, as omc_price_american_jump has it)
double drift_of(const omc_params* p, const omc_jump* j, double q, const JumpTable& t)
{
    return j->lambda == 0.0 ? p->r - q : t.drift_rate;
}

}  // namespace

extern "C" int omc_jump_paths_f32(omc_ctx* c, const omc_params* p, const omc_jump* j, double q, float* S, float* V, int64_t ld)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    JumpTable t;
    if ((rc = compose_jump(p, j, q, &t, false, true))) return rc;
    if ((rc = check_matrix(S, ld, p->n_paths))) return rc;
    if (V && p->model != OMC_MODEL_HESTON) return fail(-7, "a variance matrix is kept under Heston only (V must be NULL).");
    const omc::JumpGen g{path_spec(c, p, drift_of(p, j, q, t), S, ld), jump_law(t, j)};
    HIP_TRY(V ? omc::launch_jump_paths_sv(c->stream, g, V) : omc::launch_jump_paths(c->stream, g));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int omc_price_american_bounds_jump(omc_ctx* c, const omc_params* p, const omc_jump* j, double q,
                                              const omc_bounds_config* cfg, const double* betas, double* betas_out,
                                              double* q_out, double* samples_out, omc_bounds* out)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!cfg || !out) return fail(-7, "null bounds config or result pointer.");
    JumpTable t;
    if ((rc = compose_jump(p, j, q, &t, false, false))) return rc;
    const bool heston = p->model == OMC_MODEL_HESTON;
    if (heston && p->heston_scheme != OMC_HESTON_REFERENCE_CLAMP && p->heston_scheme != OMC_HESTON_FULL_TRUNCATION)
        return fail(-12, "price bounds under Bates take the reference or the full-truncation scheme, not the calibrator's or QE.");
    if (cfg->regressors != 0) return fail(-4, "the jump-diffusion bounds take a policy on the spot alone (regressors 0).");
    const double rj = drift_of(p, j, q, t);
    const omc::JumpLaw law = jump_law(t, j);
    omc::BoundsArgs a{};
    omc::JumpBoundsLaw l{{heston ? 1 : 0, p->heston_scheme, rj, p->sigma, p->T, p->v0, p->kappa, p->theta, p->xi, p->rho, nullptr},
                         law};
    BoundsFlow f;
    one_asset_flow(f, a, l, l.d, p, cfg);
    f.fit_paths = [&](float* S, int64_t ld) -> int {
        HIP_TRY(omc::launch_jump_paths(c->stream, omc::JumpGen{path_spec(c, p, rj, S, ld), law}));
        return 0;
    };
    f.outer = [&](hipStream_t st) {  // the outer paths: spots and, under Heston, the variance state, KEEP
        const omc::JumpGen g{path_spec(c, p, rj, (float*)a.So, a.n_outer, a.n_outer, cfg->stream_outer, 0), law};
        return heston ? omc::launch_jump_paths_sv(st, g, (float*)l.d.Vo) : omc::launch_jump_paths(st, g);
    };
    return run_bounds(c, p, cfg, betas, betas_out, q_out, samples_out, out, f);
}
