// omc_api_basket.hip -- American options on several correlated GBM assets (include/omc.h):
// arithmetic and geometric baskets, best-of and worst-of, and the running averages of the basket value (the Asian kinds,
// section 23).  The basket generator (omc_basket.hip) simulates the assets in
// registers and writes the full-storage matrix of the INDEX; the unchanged two-pass flow (enqueue_lsm) prices it, so the
// exercise policy is a function of the index alone.
#include <algorithm>

#include "omc_basket.h"
#include "omc_ctx.h"

using namespace omc::abi;

namespace omc::abi {

// The argument checks of the multi-asset entry points and the host constants, all in float64.
int compose_basket(const omc_params* p, const omc_basket* k, BasketTable* t)
{
    int rc;
    if (!p) return fail(-7, "null params.");
    if (p->model != OMC_MODEL_GBM) return fail(-12, "multi-asset options are available for GBM only.");
    if (!k) return fail(-29, "null basket.");
    const int d = k->n_assets;
    if (d < 1 || d > omc::kBasketMax) return fail(-29, "n_assets must be in 1 .. 8.");
    for (int i = 0; i < d; ++i) {
        if (!(std::isfinite(k->S0[i]) && k->S0[i] > 0.0)) return fail(-30, "every asset's spot must be finite and positive.");
        if (!(std::isfinite(k->sigma[i]) && k->sigma[i] > 0.0)) return fail(-30, "every asset's sigma must be finite and positive.");
        if (!std::isfinite(k->q[i])) return fail(-30, "every asset's dividend yield must be finite.");
        if (!(std::isfinite(k->w[i]) && k->w[i] > 0.0)) return fail(-30, "every asset's weight must be finite and positive.");
    }
    // (the value 4 between the two families was never a kind and callers were promised -32 for it: it stays refused)
    if (k->kind < OMC_BASKET_ARITHMETIC || k->kind > OMC_BASKET_ASIAN_GEOMETRIC ||
        (k->kind > OMC_BASKET_WORST_OF && !omc::basket_kind_is_asian(k->kind)))
        return fail(-32, "unknown basket kind.");
    const double* rho = k->rho;
    for (int i = 0; i < d; ++i) {
        for (int j = 0; j < d; ++j) {
            if (!std::isfinite(rho[i * d + j])) return fail(-31, "the correlation matrix has an entry that is not finite.");
            if (std::fabs(rho[i * d + j] - rho[j * d + i]) > 1e-12) return fail(-31, "the correlation matrix is not symmetric.");
        }
        if (std::fabs(rho[i * d + i] - 1.0) > 1e-12) return fail(-31, "the correlation matrix needs a unit diagonal.");
    }
    t->d = d;
    for (int i = 0; i < d; ++i) {  // Cholesky-Banachiewicz, row by row
        double* Li = t->L + i * (i + 1) / 2;
        for (int j = 0; j <= i; ++j) {
            const double* Lj = t->L + j * (j + 1) / 2;
            double s = rho[i * d + j];
            for (int m = 0; m < j; ++m) s -= Li[m] * Lj[m];
            if (j == i) {
                if (!(s > 1e-12)) return fail(-31, "the correlation matrix is not positive definite.");
                Li[j] = std::sqrt(s);
            } else {
                Li[j] = s / Lj[j];
            }
        }
    }
    // the index of the initial spots, and the geometric basket's own GBM
    double arith = 0.0, best = 0.0, worst = 0.0, G0 = 1.0, var = 0.0, drift = 0.0;
    for (int i = 0; i < d; ++i) {
        const double ws = k->w[i] * k->S0[i];
        arith += ws;
        best = i == 0 ? ws : std::max(best, ws);
        worst = i == 0 ? ws : std::min(worst, ws);
        G0 *= std::pow(k->S0[i], k->w[i]);
        for (int j = 0; j < d; ++j) var += k->w[i] * k->w[j] * k->sigma[i] * k->sigma[j] * rho[i * d + j];
        drift += k->w[i] * (p->r - k->q[i] - k->sigma[i] * k->sigma[i] / 2.0);
    }
    t->G0 = G0;
    t->sigma_G = std::sqrt(var);
    t->q_G = p->r - drift - var / 2.0;
    // (the running averages start at the basket value: X_0 = B_0)
    t->x0 = k->kind == OMC_BASKET_ARITHMETIC || omc::basket_kind_is_asian(k->kind) ? arith
            : k->kind == OMC_BASKET_GEOMETRIC ? G0 : k->kind == OMC_BASKET_BEST_OF ? best : worst;
    if (!(std::isfinite(t->x0) && t->x0 > 0.0 && (float)t->x0 > 0.0f && std::isfinite((float)t->x0)))
        return fail(-30, "the index of the initial spots must be a positive float32.");
    omc_params c = *p;  // the omc_params checks, with the index in the place of the single stock
    c.S0 = t->x0;
    c.sigma = k->sigma[0];
    if ((rc = check_params(&c))) return rc;
    if (!p->antithetic) return fail(-24, "multi-asset paths are antithetic pairs (antithetic = 1).");
    if (p->semantics != OMC_SEM_TWO_PASS) return fail(-11, "multi-asset options are priced by the two-pass flow (semantics 2).");
    const uint64_t lim = (uint64_t)1 << 40, pairs = (uint64_t)(p->n_paths / 2);
    if (p->pair_offset > lim || pairs > lim - p->pair_offset)
        return fail(-33, "pair_offset + n_paths / 2 must not exceed 2^40 (the asset tag sits above it).");
    for (int i = 0; i < d; ++i)  // (the rate: one float64 subtraction, as omc_price_american_div forms its own)
        omc::gbm_step_constants(p->r - k->q[i], k->sigma[i], p->T, p->n_steps, &t->a[i], &t->b[i]);
    return 0;
}

omc::BasketLaw basket_law(const BasketTable& t, const omc_basket* k)
{
    omc::BasketLaw law{};
    for (int i = 0; i < t.d; ++i) {
        law.a[i] = t.a[i];
        law.b[i] = t.b[i];
        law.w[i] = (float)k->w[i];
        law.s0[i] = (float)k->S0[i];
    }
    for (int i = 0; i < t.d * (t.d + 1) / 2; ++i) law.L[i] = (float)t.L[i];
    law.g0 = (float)t.G0;
    law.kind = k->kind;
    return law;
}

}  // namespace omc::abi

extern "C" {

int omc_basket_table(const omc_params* p, const omc_basket* b, double* L_packed, float* a, float* b_out, double* x0, double* geo)
{
    BasketTable t;
    int rc;
    if ((rc = compose_basket(p, b, &t))) return rc;
    if (L_packed) memcpy(L_packed, t.L, sizeof(double) * (size_t)(t.d * (t.d + 1) / 2));
    if (a) memcpy(a, t.a, sizeof(float) * (size_t)t.d);
    if (b_out) memcpy(b_out, t.b, sizeof(float) * (size_t)t.d);
    if (x0) *x0 = t.x0;
    if (geo) {
        geo[0] = t.G0;
        geo[1] = t.sigma_G;
        geo[2] = t.q_G;
    }
    return 0;
}

int omc_price_american_basket(omc_ctx* c, const omc_params* p, const omc_basket* b, omc_basket_result* out, float* S_keep,
                              float* assets_keep, int64_t ld)
{
    int rc;
    if ((rc = (S_keep || assets_keep) ? bind_in(c) : bind(c))) return rc;
    if (!out) return fail(-7, "null result pointer.");
    BasketTable t;
    if ((rc = compose_basket(p, b, &t))) return rc;
    if (c->distributed()) return fail(-10, "multi-asset pricing runs on one GPU.");
    if (assets_keep && ld < p->n_paths) return fail(-6, "leading dimension smaller than n_paths.");
    float* S;
    int64_t ld_index = ld;  // (the library's own index matrix has its own leading dimension)
    if ((rc = take_full_matrix(c, p, S_keep, &S, &ld_index))) return rc;
    memset(out, 0, sizeof *out);
    out->index0 = t.x0;
    out->n_assets = t.d;
    out->kind = b->kind;
    omc::BasketGen g{};
    g.paths = path_spec(c, p, p->r, S, ld_index);
    g.d = t.d;
    g.law = basket_law(t, b);
    g.assets = assets_keep; g.ld_assets = ld;
    if ((rc = enqueue_generated(c, p, S, ld_index, [&](hipStream_t st) { return omc::launch_basket_paths(st, g); }))) return rc;
    if ((rc = finish_generated(c, p, &out->base))) return rc;
    out->ms_basket_paths = out->base.ms_paths;
    return 0;
}

}  // extern "C"
