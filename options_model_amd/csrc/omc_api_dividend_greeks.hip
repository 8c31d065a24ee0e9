// omc_api_dividend_greeks.hip -- frozen-policy pathwise Greeks of American options on a stock that pays dividends
// (include/omc_dividend_greeks.h).  omc_price_american_div's schedule, generator and pass 1 give
// the policy -- or the caller does -- then ONE sweep (omc_dividend_greeks.hip) regenerates the paths, prices the base,
// S0 (1 + h) and S0 (1 - h) scenarios with the frozen fits and forms every Greek term.  It replaces pass 2: counts are
// those of omc_price_american_div and the price differs only in the order of its float64 sum.
#include <vector>

#include "../../include/omc_dividend_greeks.h"
#include "omc_ctx.h"
#include "omc_dividend_greeks.h"

using namespace omc::abi;

extern "C" int omc_price_american_div_greeks(omc_ctx* c, const omc_params* p, double q, const omc_dividend* d, int n_div,
                                             double bump, const double* betas, double* betas_out, omc_div_greeks* out)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!out) return fail(-7, "null result pointer.");
    // the pricing's own checks, codes and per-step table (omc_dividend_schedule; sizes first: the table has n_steps + 1 rows)
    if ((rc = check_params(p))) return rc;
    const int N = p->n_steps;
    const int64_t M = p->n_paths;
    std::vector<float> mul((size_t)N + 1), cash((size_t)N + 1);
    std::vector<int32_t> has((size_t)N + 1);
    if ((rc = omc_dividend_schedule(p, q, d, n_div, mul.data(), cash.data(), has.data()))) return rc;
    if (!(bump > 0.0 && bump <= 0.5)) return fail(-4, "bump must lie in (0, 0.5].");
    if (c->distributed()) return fail(-10, "the dividend Greeks sweep runs on one GPU.");

    // the dividend steps in step order + the closing entry; the image outlives the asynchronous copy (h_table).  A call
    // without a dividend holds the closing entry alone: the generator then writes the vanilla matrix at rate r - q.
    size_t n_ent = 0;
    for (int k = 1; k <= N; ++k) n_ent += has[(size_t)k] ? 1 : 0;
    c->h_table.resize(sizeof(omc::DivEntry) * (n_ent + 1));
    omc::DivEntry* tab = (omc::DivEntry*)c->h_table.data();
    int first = 0;
    for (int k = 1, j = 0; k <= N; ++k) {
        if (!has[(size_t)k]) continue;
        if (!first) first = k;
        tab[j++] = omc::DivEntry{k, mul[(size_t)k], cash[(size_t)k], 0};
    }
    tab[n_ent] = omc::DivEntry{omc::kDivNoStep, 1.0f, 0.0f, 0};
    if ((rc = c->div_tab.ensure(c->h_table.size()))) return rc;

    float* S = nullptr;
    int64_t ld = 0;
    if (!betas && (rc = take_full_matrix(c, p, nullptr, &S, &ld))) return rc;  // the caller's fits need no matrix
    omc::LsmWorkspace w;
    if ((rc = prepare_lsm(c, M, N, p->r, p->T, betas == nullptr, betas_out != nullptr, &w))) return rc;
    if (betas && (rc = upload_fits(c, w, betas, N))) return rc;

    const omc::DividendGen gen{path_spec(c, p, p->r - q, S, ld), (const omc::DivEntry*)c->div_tab.p};
    omc::DivGreeksArgs g{};
    g.paths = gen.paths;
    g.tab = gen.tab;
    g.is_put = p->is_put ? 1 : 0;
    g.K = p->K; g.r = p->r; g.q = q; g.h = bump;
    g.D = w.D; g.betas = w.betas; g.gmom = betas ? nullptr : w.gmom;
    const int64_t nwg = omc::dividend_greeks_blocks(M);
    if ((rc = c->gk_part.ensure(sizeof(double) * omc::kGreeksQ * (size_t)nwg))) return rc;
    if ((rc = c->gk_res.ensure(sizeof(double) * omc::kGreeksQ))) return rc;
    g.part = (double*)c->gk_part.p;
    g.result = (double*)c->gk_res.p;

    omc::LsmProblem prob{S, ld, M, N, g.is_put, p->K, p->r, p->T};
    w.ev_p1_end = c->ev[4];
    // (the table's copy stays ahead of event 0: ms_div_paths is the generator alone)
    HIP_TRY(hipMemcpyAsync(c->div_tab.p, tab, c->h_table.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    if (!betas) HIP_TRY(omc::launch_dividend_paths(c->stream, gen));
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    const bool fit = betas == nullptr && N >= 2;
    if (fit) {
        HIP_TRY(omc::lsm_pass1_moments(c->stream, prob, w));
        HIP_TRY(omc::lsm_solve_betas(c->stream, w.gmom, w.betas, N));
    }
    HIP_TRY(omc::dividend_greeks(c->stream, g, c->ev[5], c->ev[6]));
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    double h[omc::kGreeksQ];
    HIP_TRY(hipMemcpyAsync(h, g.result, sizeof h, hipMemcpyDeviceToHost, c->stream));
    if (betas_out) {
        if (betas) memcpy(betas_out, betas, sizeof(double) * 4 * (size_t)(N + 1));
        else HIP_TRY(hipMemcpyAsync(betas_out, w.betas, sizeof(double) * 4 * (size_t)(N + 1), hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = wait_stream(c))) return rc;

    memset(out, 0, sizeof *out);
    omc_greeks* o = &out->g;
    if (!fit) h[4] = 0.0;  // (no pass 1: the moment table was not written)
    fill_result(&o->base, h, M);
    o->base.folded = 0;
    const double Md = (double)M;
    mean_and_se(h[8], h[9], Md, &o->delta, &o->se_delta);
    mean_and_se(h[10], h[11], Md, &o->gamma, &o->se_gamma);
    if (p->model == OMC_MODEL_GBM) {
        mean_and_se(h[12], h[13], Md, &o->vega, &o->se_vega);
        mean_and_se(h[14], h[15], Md, &o->rho, &o->se_rho);
        mean_and_se(h[16], h[17], Md, &o->theta, &o->se_theta);
        mean_and_se(h[20], h[21], Md, &out->epsilon, &out->se_epsilon);
    } else {  // the sweep carries no tangent to the variance path's parameters
        o->vega = o->rho = o->theta = out->epsilon = NAN;
        o->se_vega = o->se_rho = o->se_theta = out->se_epsilon = NAN;
    }
    o->bump = bump;
    o->price_up = h[5] / Md;
    o->price_down = h[6] / Md;
    o->n_exercised_up = (int64_t)llround(h[18]);
    o->n_exercised_down = (int64_t)llround(h[19]);
    out->n_div_steps = (int32_t)n_ent;
    out->first_div_step = first;
    // no pass 2 (ev[5] .. ev[6] is the Greeks sweep), and with the caller's fits neither paths nor pass 1
    if ((rc = read_kernel_times(c->ev, nullptr, &o->base))) return rc;
    float ms = 0;
    if (fit) {
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[1], c->ev[4]));
        o->base.ms_pass1 = ms;
    }
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[5], c->ev[6]));
    o->ms_greeks = ms;
    return 0;
}
