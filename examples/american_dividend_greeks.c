/* C host for libomc.so (include/omc_dividend_greeks.h): the hedge ratios of an ATM American put on a stock that pays
 * quarterly cash dividends (S0 = K = 100, r = 0.05, T = 1; a dividend at t = 0.125, 0.375, 0.625, 0.875) on GPU 0 through
 * omc_price_american_div_greeks, beside the quote of omc_price_american_div they belong to.  The exercise policy pass 1
 * fits is held fixed; one forward sweep regenerates the paths and carries their tangents through every dividend.
 * model 0: GBM (sigma = 0.2): delta, gamma, vega, rho, theta, epsilon; model 1: Heston (v0 = theta = 0.04, kappa = 2,
 * xi = 0.3, rho = -0.7; the reference's log-Euler scheme): delta and gamma, the others are NaN.
 *
 *   gcc -O2 -I include examples/american_dividend_greeks.c -o /tmp/american_dividend_greeks \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/american_dividend_greeks [n_paths] [n_steps] [model: 0 GBM, 1 Heston] [dividend] [yield] [bump] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc_dividend_greeks.h"

int main(int argc, char** argv)
{
    const long long n_paths = argc > 1 ? atoll(argv[1]) : 1000000;
    const int n_steps = argc > 2 ? atoi(argv[2]) : 252;
    const int heston = argc > 3 ? atoi(argv[3]) : 0;
    const double amount = argc > 4 ? atof(argv[4]) : 1.0;
    const double q = argc > 5 ? atof(argv[5]) : 0.0;
    const double bump = argc > 6 ? atof(argv[6]) : 0.01;
    omc_dividend d[4];
    for (int i = 0; i < 4; ++i) {
        d[i].t = 0.125 + 0.25 * i;
        d[i].amount = amount;
        d[i].kind = OMC_DIV_CASH;
        d[i].reserved = 0;
    }
    omc_params p;
    memset(&p, 0, sizeof p);
    p.model = heston ? OMC_MODEL_HESTON : OMC_MODEL_GBM;
    p.heston_scheme = OMC_HESTON_REFERENCE_CLAMP;
    p.is_put = 1;
    p.semantics = OMC_SEM_TWO_PASS;
    p.antithetic = 1;
    p.n_paths = n_paths / 2 * 2;
    p.n_steps = n_steps;
    p.S0 = 100.0; p.K = 100.0; p.r = 0.05; p.sigma = 0.2; p.T = 1.0;
    p.v0 = 0.04; p.kappa = 2.0; p.theta = 0.04; p.xi = 0.3; p.rho = -0.7;
    p.seed = 42;
    omc_ctx* ctx = NULL;
    int rc = omc_ctx_create(0, NULL, &ctx);
    if (rc != 0) {
        fprintf(stderr, "omc_ctx_create: %d (%s)\n", rc, omc_last_error());
        return 1;
    }
    omc_div_result quote;
    rc = omc_price_american_div(ctx, &p, q, d, 4, &quote, NULL, 0);
    if (rc != 0) {
        fprintf(stderr, "omc_price_american_div: %d (%s)\n", rc, omc_last_error());
        omc_ctx_destroy(ctx);
        return 1;
    }
    omc_div_greeks out;
    rc = omc_price_american_div_greeks(ctx, &p, q, d, 4, bump, NULL, NULL, &out);
    if (rc != 0) {
        fprintf(stderr, "omc_price_american_div_greeks: %d (%s)\n", rc, omc_last_error());
        omc_ctx_destroy(ctx);
        return 1;
    }
    const omc_greeks* g = &out.g;
    printf("american %s put, %lld paths, %d steps, 4 cash dividends of %.3f, yield %.4f\n", heston ? "heston" : "gbm",
           (long long)p.n_paths, n_steps, amount, q);
    printf("price %.6f (two-pass quote %.6f), %lld paths exercised early; %d dividend steps, the first at step %d\n",
           g->base.price, quote.base.price, (long long)g->base.n_exercised, (int)out.n_div_steps, (int)out.first_div_step);
    printf("delta   %+.6f (se %.6f)\ngamma   %+.6f (se %.6f)   bump %.4f: price_up %.6f price_down %.6f\n", g->delta, g->se_delta,
           g->gamma, g->se_gamma, g->bump, g->price_up, g->price_down);
    printf("vega    %+.6f (se %.6f)\nrho     %+.6f (se %.6f)\ntheta   %+.6f (se %.6f)\nepsilon %+.6f (se %.6f)\n", g->vega,
           g->se_vega, g->rho, g->se_rho, g->theta, g->se_theta, out.epsilon, out.se_epsilon);
    printf("kernels: paths %.3f ms, pass 1 %.3f ms, greeks sweep %.3f ms (the quote: paths %.3f ms, pass 2 %.3f ms)\n",
           g->base.ms_paths, g->base.ms_pass1, g->ms_greeks, quote.ms_div_paths, quote.base.ms_pass2);
    omc_ctx_destroy(ctx);
    return 0;
}
