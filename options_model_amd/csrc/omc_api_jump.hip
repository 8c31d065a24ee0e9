// omc_api_jump.hip -- American options under jump-diffusion (include/omc.h): Merton (GBM) and
// Bates (Heston) paths with compound-Poisson lognormal jumps and a continuous dividend yield q.  The jump generator
// (omc_jump.hip) writes the full-storage matrix at the compensated drift rate; the unchanged two-pass flow
// (enqueue_lsm) prices it.  lambda = 0 is the yield-only route of omc_price_american_div.
#include <algorithm>

#include "omc_ctx.h"
#include "omc_jump.h"

using namespace omc::abi;

namespace omc::abi {

// The argument checks of the jump entry points and the host side of the jump law, all in float64 (omc_ctx.h).
int compose_jump(const omc_params* p, const omc_jump* j, double q, JumpTable* t, bool priced, bool start_state)
{
    int rc;
    omc_params chk;
    if (p && start_state && p->model == OMC_MODEL_HESTON && p->heston_scheme != OMC_HESTON_QE) {
        chk = *p;
        chk.v0 = 0.0;  // a start state is not validated: a stored full-truncation state may be negative
        rc = check_params(&chk);
    } else {
        rc = check_params(p);
    }
    if (rc) return rc;
    if (!j) return fail(-25, "null jump parameters.");
    if (!std::isfinite(q)) return fail(-17, "dividend yield q must be finite.");
    if (!(std::isfinite(j->lambda) && j->lambda >= 0.0)) return fail(-26, "jump intensity lambda must be finite and non-negative.");
    if (!std::isfinite(j->mu_j)) return fail(-27, "jump mean mu_j must be finite.");
    if (!(std::isfinite(j->sigma_j) && j->sigma_j >= 0.0)) return fail(-27, "jump volatility sigma_j must be finite and non-negative.");
    const double x = j->lambda * p->T / p->n_steps;
    if (!(x <= 1.0)) return fail(-28, "lambda * T / n_steps must not exceed 1: use more time steps.");
    if (!p->antithetic) return fail(-24, "jump paths are antithetic pairs (antithetic = 1).");
    if (priced && p->semantics != OMC_SEM_TWO_PASS)
        return fail(-11, "jump-diffusion is priced by the two-pass flow (semantics 2).");
    t->kappa = std::exp(j->mu_j + j->sigma_j * j->sigma_j / 2.0) - 1.0;
    t->drift_rate = (p->r - q) - j->lambda * t->kappa;
    double pn = std::exp(-x), cn = 0.0;
    t->n_thr = 0;
    for (int n = 0; n < omc::kJumpThr; ++n) {
        if (n > 0) pn = pn * x / n;
        cn += pn;
        t->thr[n] = (uint32_t)std::min(16777216.0, std::floor(cn * 16777216.0 + 0.5));
        t->n_thr += t->thr[n] < 16777216u ? 1 : 0;
    }
    return 0;
}

omc::JumpLaw jump_law(const JumpTable& t, const omc_jump* j)
{
    omc::JumpLaw law{};
    memcpy(law.thr, t.thr, sizeof t.thr);
    const double L2E = 1.4426950408889634074;
    law.mj2 = (float)(j->mu_j * L2E);
    law.sj2 = (float)(j->sigma_j * L2E);
    return law;
}

}  // namespace omc::abi

extern "C" {

int omc_jump_table(const omc_params* p, const omc_jump* j, double q, uint32_t thr[16], double* kappa, double* drift_rate)
{
    JumpTable t;
    int rc;
    if ((rc = compose_jump(p, j, q, &t, true, false))) return rc;
    if (thr) memcpy(thr, t.thr, sizeof t.thr);
    if (kappa) *kappa = t.kappa;
    if (drift_rate) *drift_rate = t.drift_rate;
    return 0;
}

int omc_price_american_jump(omc_ctx* c, const omc_params* p, const omc_jump* j, double q, omc_jump_result* out,
                            float* S_keep, int64_t ld)
{
    int rc;
    if ((rc = S_keep ? bind_in(c) : bind(c))) return rc;
    if (!out) return fail(-7, "null result pointer.");
    JumpTable t;
    if ((rc = compose_jump(p, j, q, &t, true, false))) return rc;
    if (c->distributed()) return fail(-10, "jump-diffusion pricing runs on one GPU.");
    memset(out, 0, sizeof *out);
    out->kappa = t.kappa;
    out->drift_rate = t.drift_rate;
    if (j->lambda == 0.0) {  // no jumps: the yield-only route of omc_price_american_div, under its storage rule
        omc_params gen = *p;
        gen.r = p->r - q;
        if ((rc = price_fused(c, p, &gen, &out->base, S_keep, ld))) return rc;
        out->ms_jump_paths = out->base.ms_paths;
        return 0;
    }
    float* S;
    if ((rc = take_full_matrix(c, p, S_keep, &S, &ld))) return rc;
    const omc::JumpGen g{path_spec(c, p, t.drift_rate, S, ld), jump_law(t, j)};
    if ((rc = enqueue_generated(c, p, S, ld, [&](hipStream_t st) { return omc::launch_jump_paths(st, g); }))) return rc;
    if ((rc = finish_generated(c, p, &out->base))) return rc;
    out->ms_jump_paths = out->base.ms_paths;
    out->n_thresholds = t.n_thr;
    return 0;
}

}  // extern "C"
