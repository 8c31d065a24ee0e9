// omc_api_runnerup_bounds.hip -- Andersen-Broadie price bounds of best-of / worst-of options with a policy on the index and
// the runner-up (include/omc.h): omc_price_american_basket_bounds' flow (run_bounds,
// omc_api_bounds.hip) with a policy of its own -- a table [N+1][8] fitted by omc_runnerup_bounds.hip on the basket generator's
// kept asset matrices, or the caller's -- and that file's sweeps and walk.  For the Asian kinds (section 23) the second
// regressor is the current basket value and the fit, sweeps and walk are omc_asian_bounds.hip's.
#include "omc_asian_bounds.h"
#include "omc_ctx.h"
#include "omc_runnerup_bounds.h"

using namespace omc::abi;

extern "C" int omc_price_american_basket_bounds_runnerup(omc_ctx* c, const omc_params* p, const omc_basket* bk,
                                                         const omc_bounds_config* cfg, const double* betas,
                                                         double* betas_out, double* q_out, double* samples_out,
                                                         omc_basket_bounds* out)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!cfg || !out) return fail(-7, "null bounds config or result pointer.");
    BasketTable t;
    if ((rc = compose_basket(p, bk, &t))) return rc;
    if (bk->kind == OMC_BASKET_GEOMETRIC)
        return fail(-34, "the geometric index is one GBM: ask for its bounds with one asset (G0, sigma_G, q_G of omc_basket_table).");
    // the Asian kinds (section 23): the second regressor is the current basket value, any asset count
    const bool asian = omc::basket_kind_is_asian(bk->kind);
    if (!asian && (bk->kind == OMC_BASKET_ARITHMETIC || t.d < 2))
        return fail(-35, "the runner-up policy is for best-of and worst-of options on 2 .. 8 assets.");
    if (cfg->policy == OMC_SEM_REFERENCE || cfg->policy == OMC_SEM_TWO_PASS)
        return fail(-4, "the runner-up policy is fitted by textbook Longstaff-Schwartz (policy textbook) or given.");
    const int N = p->n_steps;
    if (N > omc::kRunnerupMaxSteps) return fail(-16, "the runner-up policy takes at most 512 dates.");
    omc::RunnerupArgs g{};
    g.g.law = basket_law(t, bk);  // the generator's constants, so every spot is the generator's
    g.g.d = t.d;
    omc::BasketGen gen{};
    gen.d = t.d;
    gen.law = g.g.law;
    const bool fitted = cfg->policy != OMC_POLICY_GIVEN;
    const int64_t ld_fit = padded_ld(p->n_paths);  // ensure_paths' leading dimension of the fitting paths
    const size_t pol_bytes = sizeof(double) * omc::kRunnerupCols * (size_t)(N + 1);
    // the flow's room: outer asset matrices | asset matrices of the fitting paths | the policy | the fit's partial sums
    // (the Asian kinds: the outer running state is one more matrix behind the outer asset matrices)
    size_t o_fit = 0, o_pol = 0, o_part = 0, outer_mat = 0;
    BoundsFlow f;
    f.d = t.d;
    if (cfg->n_outer > 0) {  // (sizes are checked in run_bounds, before the room is used)
        outer_mat = (size_t)(N + 1) * (size_t)cfg->n_outer;
        o_fit = up256(sizeof(float) * (size_t)(t.d + (asian ? 1 : 0)) * outer_mat);
        o_pol = o_fit + (fitted ? up256(sizeof(float) * (size_t)t.d * (size_t)(N + 1) * (size_t)ld_fit) : 0);
        o_part = o_pol + up256(pol_bytes);
        f.extra_bytes = o_part + sizeof(double) * omc::kRunnerupSlots * omc::kRunnerupFitBlocks;
    }
    char* room = nullptr;
    f.bind = [&](const omc::BoundsArgs& common, char* extra) {
        g.g.v = common;
        g.g.Ao = (const float*)extra;
        g.g.Co = asian ? g.g.Ao + (size_t)t.d * outer_mat : nullptr;
        g.pol = (const double*)(extra + o_pol);
        room = extra;
    };
    f.own_policy = [&](const omc::LsmWorkspace& w, float* S, int64_t ld) -> int {
        double* pol = (double*)(room + o_pol);
        if (!S) {  // the caller's table; `betas` is caller memory
            HIP_TRY(hipMemcpyAsync(pol, betas, pol_bytes, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            return 0;
        }
        if (ld != ld_fit) return fail(999, "the fitting paths' leading dimension changed under the runner-up fit.");
        gen.paths = path_spec(c, p, p->r, S, ld);  // the index matrix of p, and its assets
        gen.assets = (float*)(room + o_fit); gen.ld_assets = ld;
        HIP_TRY(omc::launch_basket_paths(c->stream, gen));
        if (asian) {
            omc::AsianFit fit{};
            fit.law = g.g.law; fit.d = t.d;
            fit.S = S; fit.A = gen.assets; fit.ld = ld; fit.M = p->n_paths;
            fit.N = N; fit.is_put = g.g.v.is_put; fit.K = g.g.v.K; fit.invK = g.g.v.invK;
            fit.D = w.D; fit.x_ex = w.sx; fit.tex = w.tex;
            fit.part = (double*)(room + o_part); fit.pol = pol;
            HIP_TRY(omc::asian2_fit(c->stream, fit));
            return 0;
        }
        omc::RunnerupFit fit{};
        fit.law = g.g.law; fit.d = t.d;
        fit.A = gen.assets; fit.ld = ld; fit.M = p->n_paths;
        fit.N = N; fit.is_put = g.g.v.is_put; fit.K = g.g.v.K; fit.invK = g.g.v.invK;
        fit.D = w.D; fit.x_ex = w.sx; fit.tex = w.tex;
        fit.part = (double*)(room + o_part); fit.pol = pol;
        HIP_TRY(omc::runnerup_fit(c->stream, fit));
        return 0;
    };
    f.lower = [&](hipStream_t st, double* res) { return asian ? omc::asian2_lower(st, g, res) : omc::runnerup_lower(st, g, res); };
    f.outer = [&](hipStream_t st) {  // the outer paths: index and assets, KEEP
        gen.paths = path_spec(c, p, p->r, (float*)g.g.v.So, g.g.v.n_outer);
        gen.paths.n_paths = g.g.v.n_outer; gen.paths.stream = (uint32_t)cfg->stream_outer; gen.paths.pair_offset = 0;
        gen.assets = (float*)g.g.Ao; gen.ld_assets = g.g.v.n_outer; gen.state = (float*)g.g.Co;
        return omc::launch_basket_paths(st, gen);
    };
    f.inner = [&](hipStream_t st, int64_t i0, int64_t ni) {
        return asian ? omc::asian2_inner(st, g, i0, ni) : omc::runnerup_inner(st, g, i0, ni);
    };
    f.walk = [&](hipStream_t st, double* res) { return asian ? omc::asian2_walk(st, g, res) : omc::runnerup_walk(st, g, res); };
    f.read_policy = [&](hipStream_t st, double* host) {
        return hipMemcpyAsync(host, g.pol, pol_bytes, hipMemcpyDeviceToHost, st);
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
