// omc_api_basket_greeks.hip -- frozen-policy pathwise Greeks of American options on the index of several correlated GBM
// assets (include/omc.h).  omc_price_american_basket's paths and pass 1 give the policy -- or the
// caller does -- then ONE sweep (omc_basket_greeks.hip) regenerates the assets, prices the base scenario with pass 2's
// decisions and forms every per-asset Greek term.  It replaces pass 2: counts are those of omc_price_american_basket and
// the price differs only in the order of its float64 sum.
#include <vector>

#include "omc_basket_greeks.h"
#include "omc_ctx.h"

using namespace omc::abi;

extern "C" int omc_price_american_basket_greeks(omc_ctx* c, const omc_params* p, const omc_basket* bk, double bump,
                                                int want_gamma, const double* betas, double* betas_out,
                                                omc_basket_greeks* out)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!out) return fail(-7, "null result pointer.");
    BasketTable t;
    if ((rc = compose_basket(p, bk, &t))) return rc;
    if (omc::basket_kind_is_asian(bk->kind))  // the regenerated-asset sweep carries no running state
        return fail(-32, "the multi-asset Greeks take no running-average (Asian) kind.");
    if (!(bump > 0.0 && bump <= 0.5)) return fail(-4, "bump must lie in (0, 0.5].");
    if (c->distributed()) return fail(-10, "the multi-asset Greeks sweep runs on one GPU.");
    const int64_t M = p->n_paths;
    const int N = p->n_steps, d = t.d;
    float* S = nullptr;
    int64_t ld = 0;
    if (!betas && (rc = take_full_matrix(c, p, nullptr, &S, &ld))) return rc;
    omc::LsmWorkspace w;
    if ((rc = prepare_lsm(c, M, N, p->r, p->T, betas == nullptr, betas_out != nullptr, &w))) return rc;
    if (betas && (rc = upload_fits(c, w, betas, N))) return rc;

    omc::BasketGen gen{};
    gen.paths = path_spec(c, p, p->r, S, ld);
    gen.d = d;
    gen.law = basket_law(t, bk);
    omc::BasketGreeksArgs g{};
    g.P = M / 2; g.N = N; g.d = d; g.is_put = p->is_put ? 1 : 0; g.want_gamma = want_gamma ? 1 : 0;
    g.k0 = (uint32_t)p->seed; g.k1 = (uint32_t)(p->seed >> 32); g.stream = (uint32_t)p->stream; g.pair_offset = p->pair_offset;
    g.K = p->K; g.invK = 1.0 / p->K; g.r = p->r; g.T = p->T; g.h = bump; g.lup = 1.0 + bump; g.ldn = 1.0 - bump;
    for (int i = 0; i < d; ++i) {
        const double wf = (double)gen.law.w[i];
        g.S0[i] = bk->S0[i]; g.sigma[i] = bk->sigma[i]; g.q[i] = bk->q[i];
        g.hw[i] = bump * wf; g.cup[i] = std::pow(g.lup, wf); g.cdn[i] = std::pow(g.ldn, wf);
    }
    g.D = w.D; g.betas = w.betas;
    const int64_t nwg = omc::basket_greeks_blocks(g.P);
    const int nq = 8 * omc::basket_greeks_groups(d);
    if ((rc = c->gk_part.ensure(sizeof(double) * (size_t)nq * (size_t)nwg))) return rc;
    if ((rc = c->gk_res.ensure(sizeof(double) * (size_t)nq))) return rc;
    g.part = (double*)c->gk_part.p;
    g.result = (double*)c->gk_res.p;

    omc::LsmProblem prob{S, ld, M, N, g.is_put, p->K, p->r, p->T};
    w.ev_p1_end = c->ev[4];
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    if (!betas) HIP_TRY(omc::launch_basket_paths(c->stream, gen));
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    const bool fit = betas == nullptr && N >= 2;
    if (fit) {
        HIP_TRY(omc::lsm_pass1_moments(c->stream, prob, w));
        HIP_TRY(omc::lsm_solve_betas(c->stream, w.gmom, w.betas, N));
    }
    HIP_TRY(omc::basket_greeks(c->stream, g, gen.law, c->ev[5], c->ev[6]));
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    double h[omc::kBasketGreeksMaxQ];
    HIP_TRY(hipMemcpyAsync(h, g.result, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, c->stream));
    std::vector<double> fits;  // the fitted table: its column n gives sum_nitm
    if (fit) {
        fits.resize(4 * (size_t)(N + 1));
        HIP_TRY(hipMemcpyAsync(fits.data(), w.betas, sizeof(double) * fits.size(), hipMemcpyDeviceToHost, c->stream));
    }
    if (betas_out) {
        if (betas) memcpy(betas_out, betas, sizeof(double) * 4 * (size_t)(N + 1));
        else HIP_TRY(hipMemcpyAsync(betas_out, w.betas, sizeof(double) * 4 * (size_t)(N + 1), hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = wait_stream(c))) return rc;

    memset(out, 0, sizeof *out);
    double base[8] = {h[0], h[1], h[2], h[3], 0.0, 0.0, 0.0, 0.0};
    for (int s = 1; fit && s < N; ++s) base[4] += fits[4 * (size_t)s + 3];
    fill_result(&out->base.base, base, M);
    out->base.index0 = t.x0;
    out->base.n_assets = d;
    out->base.kind = bk->kind;
    const double Md = (double)M;
    mean_and_se(h[4], h[5], Md, &out->rho, &out->se_rho);
    mean_and_se(h[6], h[7], Md, &out->theta, &out->se_theta);
    for (int i = 0; i < d; ++i) {
        const double* a = h + 8 * (1 + i);
        mean_and_se(a[0], a[1], Md, &out->delta[i], &out->se_delta[i]);
        mean_and_se(a[2], a[3], Md, &out->vega[i], &out->se_vega[i]);
        if (g.want_gamma) {
            mean_and_se(a[4], a[5], Md, &out->gamma[i], &out->se_gamma[i]);
            out->price_up[i] = a[6] / Md;
            out->price_down[i] = a[7] / Md;
            out->n_exercised_up[i] = (int64_t)llround(h[8 * (1 + d) + 2 * i]);
            out->n_exercised_down[i] = (int64_t)llround(h[8 * (1 + d) + 2 * i + 1]);
        } else {
            out->gamma[i] = out->se_gamma[i] = out->price_up[i] = out->price_down[i] = NAN;
        }
    }
    out->bump = bump;
    out->gamma_on = g.want_gamma;
    // no pass 2 (ev[5] .. ev[6] is the Greeks sweep), and with the caller's fits neither paths nor pass 1
    if ((rc = read_kernel_times(c->ev, nullptr, &out->base.base))) return rc;
    out->base.ms_basket_paths = out->base.base.ms_paths;
    float ms = 0;
    if (fit) {
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[1], c->ev[4]));
        out->base.base.ms_pass1 = ms;
    }
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[5], c->ev[6]));
    out->ms_greeks = ms;
    return 0;
}
