/* C host for libomc.so (include/omc_barrier_bounds.h): Andersen-Broadie bounds on the value of an American down-and-out
 * ATM put (S0 = K = 100, r = 0.05, T = 1, barrier H monitored on every step of the grid, no rebate) on GPU 0 through
 * omc_price_american_bounds_barrier, beside the two-pass quote of omc_price_barrier that they bracket.  model 0: GBM
 * (sigma = 0.2); model 1: Heston (v0 = theta = 0.04, kappa = 2, xi = 0.3, rho = -0.7; the reference's log-Euler scheme).
 * The textbook Longstaff-Schwartz policy -- a function of the encoded index: the spot while the option is live -- is fitted
 * on the 100,000 encoded paths the quote is priced on (seed 42, stream 0; lower / outer / inner paths on streams 1 / 2 / 3).
 * The inner simulations start at the outer paths' (spot, knocked yes / no[, variance]) state; a knocked-out path stops.
 *
 *   gcc -O2 -I include examples/barrier_bounds.c -o /tmp/barrier_bounds \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/barrier_bounds [n_steps] [n_lower] [n_outer] [n_inner] [model: 0 GBM, 1 Heston] [H] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc_barrier_bounds.h"

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
    omc_barrier b;
    memset(&b, 0, sizeof b);
    b.kind = OMC_BARRIER_DOWN_OUT;
    b.monitoring = OMC_MONITOR_DISCRETE;
    b.american = 1;
    b.H = argc > 6 ? atof(argv[6]) : 90.0;
    omc_params p;
    memset(&p, 0, sizeof p);
    p.model = heston ? OMC_MODEL_HESTON : OMC_MODEL_GBM;
    p.heston_scheme = OMC_HESTON_REFERENCE_CLAMP;
    p.is_put = 1;
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
    omc_barrier_result quote;
    rc = omc_price_barrier(ctx, &p, &b, &quote, NULL, 0);
    if (rc != 0) {
        fprintf(stderr, "omc_price_barrier: %d (%s)\n", rc, omc_last_error());
        omc_ctx_destroy(ctx);
        return 1;
    }
    omc_bounds out;
    rc = omc_price_american_bounds_barrier(ctx, &p, &b, &cfg, NULL, NULL, NULL, NULL, &out);
    if (rc != 0) {
        fprintf(stderr, "omc_price_american_bounds_barrier: %d (%s)\n", rc, omc_last_error());
        omc_ctx_destroy(ctx);
        return 1;
    }
    printf("american %s down-and-out put, %d dates, H = %.3f: bounds [%.6f, %.6f]  se %.6f / %.6f  95%% interval [%.6f, %.6f]\n",
           heston ? "heston" : "gbm", n_steps, b.H, out.lower, out.upper, out.se_lower, out.se_upper, out.ci_lo, out.ci_hi);
    printf("two-pass quote %.6f (European knock-out %.6f, %.1f%% of the paths hit)\n", quote.base.price, quote.euro_out,
           100.0 * quote.hit_prob);
    printf("lower: %lld paths, %lld stopped before maturity; upper: %lld outer x %lld inner, inner path-steps %lld\n",
           (long long)out.n_lower, (long long)out.n_exercised_lower, (long long)out.n_outer, (long long)out.n_inner,
           (long long)out.inner_path_steps);
    printf("kernels: fit %.3f ms, lower %.3f ms, upper %.3f ms, total %.3f ms\n", out.ms_fit, out.ms_lower, out.ms_upper,
           out.ms_total);
    omc_ctx_destroy(ctx);
    return 0;
}
