// omc_api_basket_bounds.hip -- Andersen-Broadie price bounds of American options on the index of several correlated GBM
// assets (include/omc.h): omc_price_american_bounds' flow (run_bounds, omc_api_bounds.hip) with the
// basket generator writing the matrices and the multi-asset kernels of omc_basket_bounds.hip simulating the fresh paths.
// For the Asian kinds (section 23) the outer generator also stores the running state, which the inner paths start from.
#include "omc_basket_bounds.h"
#include "omc_ctx.h"

using namespace omc::abi;

extern "C" int omc_price_american_basket_bounds(omc_ctx* c, const omc_params* p, const omc_basket* bk,
                                                const omc_bounds_config* cfg, const double* betas, double* betas_out,
                                                double* q_out, double* samples_out, omc_basket_bounds* out)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!cfg || !out) return fail(-7, "null bounds config or result pointer.");
    BasketTable t;
    if ((rc = compose_basket(p, bk, &t))) return rc;
    if (bk->kind == OMC_BASKET_GEOMETRIC)
        return fail(-34, "the geometric index is one GBM: ask for its bounds with one asset (G0, sigma_G, q_G of omc_basket_table).");
    omc::BasketBoundsArgs g{};
    g.law = basket_law(t, bk);  // the generator's constants, so every spot is the generator's
    g.d = t.d;
    omc::BasketGen gen{};
    gen.d = t.d;
    gen.law = g.law;
    BoundsFlow f;
    f.d = t.d;
    // the Asian kinds keep the outer running state, one more matrix behind the outer asset matrices: the inner paths start there
    const bool asian = omc::basket_kind_is_asian(bk->kind);
    const size_t outer_mat = cfg->n_outer > 0 ? (size_t)(p->n_steps + 1) * (size_t)cfg->n_outer : 0;  // floats of one matrix
    if (cfg->n_outer > 0)  // (sizes are checked in run_bounds, before the room is used)
        f.extra_bytes = sizeof(float) * (size_t)(t.d + (asian ? 1 : 0)) * outer_mat;
    f.fit_paths = [&](float* S, int64_t ld) {  // the index matrix of p
        gen.paths = path_spec(c, p, p->r, S, ld);
        HIP_TRY(omc::launch_basket_paths(c->stream, gen));
        return 0;
    };
    f.bind = [&](const omc::BoundsArgs& common, char* extra) {
        g.v = common;
        g.Ao = (const float*)extra;
        g.Co = asian ? g.Ao + (size_t)t.d * outer_mat : nullptr;
    };
    f.lower = [&](hipStream_t st, double* res) { return omc::basket_bounds_lower(st, g, res); };
    f.outer = [&](hipStream_t st) {  // the outer paths: index and assets, KEEP
        gen.paths = path_spec(c, p, p->r, (float*)g.v.So, g.v.n_outer);
        gen.paths.n_paths = g.v.n_outer; gen.paths.stream = (uint32_t)cfg->stream_outer; gen.paths.pair_offset = 0;
        gen.assets = (float*)g.Ao; gen.ld_assets = g.v.n_outer; gen.state = (float*)g.Co;
        return omc::launch_basket_paths(st, gen);
    };
    f.inner = [&](hipStream_t st, int64_t i0, int64_t ni) { return omc::basket_bounds_inner(st, g, i0, ni); };
    f.inner_check = [&](hipStream_t st, const omc::BoundsCheck& k, int64_t i0, int64_t ni) {  // section 27: the payoff check
        return omc::basket_bounds_check_inner(st, g, k, i0, ni);
    };
    omc_bounds bounds;
    if ((rc = run_bounds(c, p, cfg, betas, betas_out, q_out, samples_out, &bounds, f))) return rc;
    memset(out, 0, sizeof *out);
    out->bounds = bounds;
    out->index0 = t.x0;
    out->n_assets = t.d;
    out->kind = bk->kind;
    return 0;
}
