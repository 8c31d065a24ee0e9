/* C host for libomc.so (include/omc.h): the price bracket of the ATM GBM put (S0 = K = 100, r = 0.05, sigma = 0.2, T = 1,
 * exercisable at each of 50 dates) on GPU 0 through omc_price_american_bounds, first plain and then with option
 * "bounds_control_variate" = 1 -- the discounted Black-Scholes value of the European put as a control variate in the lower
 * bound and in every inner mean -- at a sixteenth of the inner paths.  The paths and the stops are the same in both calls with
 * the same n_inner; the controlled bracket is the tighter one, on far less inner work.  Textbook Longstaff-Schwartz policy
 * fitted on 100,000 paths (seed 42, stream 0; lower / outer / inner paths on streams 1 / 2 / 3).
 *
 *   gcc -O2 -I include examples/american_bounds_cv.c -o /tmp/american_bounds_cv \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/american_bounds_cv [n_steps] [n_lower] [n_outer] [n_inner plain] [n_inner controlled] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc.h"

int main(int argc, char** argv)
{
    omc_bounds_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.policy = OMC_SEM_TEXTBOOK;
    cfg.n_lower = argc > 2 ? atoll(argv[2]) : 1000000;
    cfg.n_outer = argc > 3 ? atoll(argv[3]) : 8192;
    const long long n_inner[2] = {argc > 4 ? atoll(argv[4]) : 1024, argc > 5 ? atoll(argv[5]) : 64};
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
    p.n_steps = argc > 1 ? atoi(argv[1]) : 50;
    p.S0 = 100.0; p.K = 100.0; p.r = 0.05; p.sigma = 0.2; p.T = 1.0;
    p.seed = 42;
    omc_ctx* ctx = NULL;
    int rc = omc_ctx_create(0, NULL, &ctx);
    if (rc != 0) {
        fprintf(stderr, "omc_ctx_create: %d (%s)\n", rc, omc_last_error());
        return 1;
    }
    const char* name[2] = {"plain", "controlled"};
    for (int v = 0; v < 2; ++v) {
        rc = omc_set_option(ctx, "bounds_control_variate", v);
        if (rc != 0) {
            fprintf(stderr, "omc_set_option: %d (%s)\n", rc, omc_last_error());
            omc_ctx_destroy(ctx);
            return 1;
        }
        cfg.n_inner = n_inner[v];
        omc_bounds out;
        rc = omc_price_american_bounds(ctx, &p, &cfg, NULL, NULL, NULL, NULL, &out);
        if (rc != 0) {
            fprintf(stderr, "omc_price_american_bounds: %d (%s)\n", rc, omc_last_error());
            omc_ctx_destroy(ctx);
            return 1;
        }
        printf("%s put, control_variate %d, n_inner %lld: bounds [%.6f, %.6f]  se %.6f / %.6f  inner path-steps %lld  "
               "total %.3f ms\n", name[v], v, n_inner[v], out.lower, out.upper, out.se_lower, out.se_upper,
               (long long)out.inner_path_steps, out.ms_total);
    }
    omc_set_option(ctx, "bounds_control_variate", 0); /* the context's default again */
    omc_ctx_destroy(ctx);
    return 0;
}
