/* C host for libomc.so (include/omc_dividend_bounds.h): Andersen-Broadie bounds on the Bermudan value of an ATM call on a
 * stock that pays quarterly cash dividends (S0 = K = 100, r = 0.05, T = 1; a dividend at t = 0.125, 0.375, 0.625, 0.875) on
 * GPU 0 through omc_price_american_bounds_div, beside the quote of omc_price_american_div that they bracket.  Early exercise
 * of a call pays only just before a dividend: exercising at an ex-dividend step earns the ex-dividend payoff, the last
 * cum-dividend date is the step before.  model 0: GBM (sigma = 0.2); model 1: Heston (v0 = theta = 0.04, kappa = 2,
 * xi = 0.3, rho = -0.7; the reference's log-Euler scheme).  The textbook Longstaff-Schwartz policy -- a function of the
 * spot alone -- is fitted on 100,000 dividend paths (seed 42, stream 0; lower / outer / inner paths on streams 1 / 2 / 3).
 * The inner simulations start at the outer paths' spot (GBM) or (spot, variance) state (Heston) and at their date.
 *
 *   gcc -O2 -I include examples/american_dividend_bounds.c -o /tmp/american_dividend_bounds \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/american_dividend_bounds [n_steps] [n_lower] [n_outer] [n_inner] [model: 0 GBM, 1 Heston] [dividend] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc_dividend_bounds.h"

int main(int argc, char** argv)
{
    const int n_steps = argc > 1 ? atoi(argv[1]) : 50;
    omc_bounds_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.policy = OMC_SEM_TEXTBOOK;
    cfg.n_lower = argc > 2 ? atoll(argv[2]) : 1000000;
    cfg.n_outer = argc > 3 ? atoll(argv[3]) : 8192;
    cfg.n_inner = argc > 4 ? atoll(argv[4]) : 1024;
    cfg.stream_lower = 1;
    cfg.stream_outer = 2;
    cfg.stream_inner = 3;
    const int heston = argc > 5 ? atoi(argv[5]) : 0;
    const double amount = argc > 6 ? atof(argv[6]) : 1.0;
    const double q = 0.0;
    omc_dividend d[4];
    for (int i = 0; i < 4; ++i) {
        d[i].t = 0.125 + 0.25 * i;
        d[i].amount = amount;
        d[i].kind = OMC_DIV_CASH;
    }
    omc_params p;
    memset(&p, 0, sizeof p);
    p.model = heston ? OMC_MODEL_HESTON : OMC_MODEL_GBM;
    p.heston_scheme = OMC_HESTON_REFERENCE_CLAMP;
    p.is_put = 0;
    p.semantics = OMC_SEM_TWO_PASS; /* the quote's flow; the bounds do not use it: cfg.policy chooses the fits */
    p.antithetic = 1;
    p.n_paths = 100000;
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
    omc_bounds out;
    rc = omc_price_american_bounds_div(ctx, &p, q, d, 4, &cfg, NULL, NULL, NULL, NULL, &out);
    if (rc != 0) {
        fprintf(stderr, "omc_price_american_bounds_div: %d (%s)\n", rc, omc_last_error());
        omc_ctx_destroy(ctx);
        return 1;
    }
    printf("bermudan %s call, %d dates, 4 cash dividends of %.3f: bounds [%.6f, %.6f]  se %.6f / %.6f  95%% interval [%.6f, %.6f]\n",
           heston ? "heston" : "gbm", n_steps, amount, out.lower, out.upper, out.se_lower, out.se_upper, out.ci_lo, out.ci_hi);
    printf("two-pass quote %.6f (%d dividend steps, the first at step %d)\n", quote.base.price, (int)quote.n_div_steps,
           (int)quote.first_div_step);
    printf("lower: %lld paths, %lld stopped before maturity; upper: %lld outer x %lld inner, inner path-steps %lld\n",
           (long long)out.n_lower, (long long)out.n_exercised_lower, (long long)out.n_outer, (long long)out.n_inner,
           (long long)out.inner_path_steps);
    printf("kernels: fit %.3f ms, lower %.3f ms, upper %.3f ms, total %.3f ms\n", out.ms_fit, out.ms_lower, out.ms_upper,
           out.ms_total);
    omc_ctx_destroy(ctx);
    return 0;
}
