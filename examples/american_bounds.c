/* C host for libomc.so (include/omc.h): Andersen-Broadie bounds on the Bermudan value of the ATM GBM put (S0 = K = 100,
 * r = 0.05, sigma = 0.2, T = 1) on GPU 0 through omc_price_american_bounds, with the textbook Longstaff-Schwartz policy
 * fitted on 100,000 paths (seed 42, stream 0; lower / outer / inner paths on streams 1 / 2 / 3).
 *
 *   gcc -O2 -I include examples/american_bounds.c -o /tmp/american_bounds \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/american_bounds [n_steps] [n_lower] [n_outer] [n_inner] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc.h"

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
    omc_params p;
    memset(&p, 0, sizeof p);
    p.model = OMC_MODEL_GBM;
    p.is_put = 1;
    p.semantics = OMC_SEM_TWO_PASS; /* not used by the bounds: cfg.policy chooses the fits */
    p.antithetic = 1;
    p.n_paths = 100000;
    p.n_steps = n_steps;
    p.S0 = 100.0; p.K = 100.0; p.r = 0.05; p.sigma = 0.2; p.T = 1.0;
    p.seed = 42;
    omc_ctx* ctx = NULL;
    int rc = omc_ctx_create(0, NULL, &ctx);
    if (rc != 0) {
        fprintf(stderr, "omc_ctx_create: %d (%s)\n", rc, omc_last_error());
        return 1;
    }
    omc_bounds out;
    rc = omc_price_american_bounds(ctx, &p, &cfg, NULL, NULL, NULL, NULL, &out);
    if (rc != 0) {
        fprintf(stderr, "omc_price_american_bounds: %d (%s)\n", rc, omc_last_error());
        omc_ctx_destroy(ctx);
        return 1;
    }
    printf("bermudan put, %d dates: bounds [%.6f, %.6f]  se %.6f / %.6f  95%% interval [%.6f, %.6f]\n", n_steps, out.lower,
           out.upper, out.se_lower, out.se_upper, out.ci_lo, out.ci_hi);
    printf("lower: %lld paths, %lld stopped before maturity; upper: %lld outer x %lld inner, inner path-steps %lld\n",
           (long long)out.n_lower, (long long)out.n_exercised_lower, (long long)out.n_outer, (long long)out.n_inner,
           (long long)out.inner_path_steps);
    printf("kernels: fit %.3f ms, lower %.3f ms, upper %.3f ms, total %.3f ms\n", out.ms_fit, out.ms_lower, out.ms_upper,
           out.ms_total);
    omc_ctx_destroy(ctx);
    return 0;
}
