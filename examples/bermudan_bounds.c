/* C host for libomc.so (include/omc.h): price brackets for ONE strike under three exercise rights on the same daily grid --
 * the ATM GBM put (S0 = K = 100, r = 0.05, sigma = 0.2, T = 1) on 252 steps, exercisable at every date (American on the
 * grid), at every 21st date counted back from expiry (a monthly Bermudan) and at expiry alone (European) -- on GPU 0 through
 * omc_price_american_bounds with option "bounds_exercise_every" = 0, 21 and n_steps.  The option changes the game whose
 * value is bounded; the paths are the daily grid's in all three.  Textbook Longstaff-Schwartz policy fitted on 100,000 paths
 * (seed 42, stream 0; lower / outer / inner paths on streams 1 / 2 / 3).
 *
 *   gcc -O2 -I include examples/bermudan_bounds.c -o /tmp/bermudan_bounds \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/bermudan_bounds [n_steps] [exercise_every] [n_lower] [n_outer] [n_inner] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc.h"

int main(int argc, char** argv)
{
    const int n_steps = argc > 1 ? atoi(argv[1]) : 252;
    const long long monthly = argc > 2 ? atoll(argv[2]) : 21;
    omc_bounds_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.policy = OMC_SEM_TEXTBOOK;
    cfg.n_lower = argc > 3 ? atoll(argv[3]) : 400000;
    cfg.n_outer = argc > 4 ? atoll(argv[4]) : 2048;
    cfg.n_inner = argc > 5 ? atoll(argv[5]) : 256;
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
    const char* name[3] = {"american", "bermudan", "european"};
    const long long every[3] = {0, monthly, n_steps};
    for (int i = 0; i < 3; ++i) {
        rc = omc_set_option(ctx, "bounds_exercise_every", every[i]);
        if (rc != 0) {
            fprintf(stderr, "omc_set_option: %d (%s)\n", rc, omc_last_error());
            omc_ctx_destroy(ctx);
            return 1;
        }
        omc_bounds out;
        rc = omc_price_american_bounds(ctx, &p, &cfg, NULL, NULL, NULL, NULL, &out);
        if (rc != 0) {
            fprintf(stderr, "omc_price_american_bounds: %d (%s)\n", rc, omc_last_error());
            omc_ctx_destroy(ctx);
            return 1;
        }
        const long long k = every[i] < 2 ? 1 : (every[i] > n_steps ? n_steps : every[i]);
        printf("%s put, exercise_every %lld (%lld dates of %d): bounds [%.6f, %.6f]  se %.6f / %.6f  inner path-steps %lld  "
               "total %.3f ms\n", name[i], every[i], (long long)((n_steps - 1) / k + 1), n_steps, out.lower, out.upper,
               out.se_lower, out.se_upper, (long long)out.inner_path_steps, out.ms_total);
    }
    omc_set_option(ctx, "bounds_exercise_every", 0); /* the context's default again */
    omc_ctx_destroy(ctx);
    return 0;
}
