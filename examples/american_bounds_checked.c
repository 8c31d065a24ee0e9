/* C host for libomc.so (include/omc.h): the price bracket of the ATM GBM put (S0 = K = 100, r = 0.05, sigma = 0.2, T = 1,
 * exercisable at each of 50 dates) on GPU 0 through omc_price_american_bounds with the Black-Scholes control variate, three
 * times: with option "bounds_suboptimality" = 0 (off), 1 (payoff) and 2 (European) -- Broadie-Cao's sub-optimality checking,
 * which runs the inner simulations only at the (outer path, date) items at which exercise is not known to be sub-optimal.
 * The lower bound is the same in all three calls; the upper bound can only fall and stays an upper bound; the inner
 * path-steps show the work that is left.  Textbook Longstaff-Schwartz policy fitted on 100,000 paths (seed 42, stream 0;
 * lower / outer / inner paths on streams 1 / 2 / 3).
 *
 *   gcc -O2 -I include examples/american_bounds_checked.c -o /tmp/american_bounds_checked \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/american_bounds_checked [n_steps] [n_lower] [n_outer] [n_inner] [control_variate] */
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
    cfg.n_inner = argc > 4 ? atoll(argv[4]) : 64;
    const int cv = argc > 5 ? atoi(argv[5]) : 1;
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
    rc = omc_set_option(ctx, "bounds_control_variate", cv);
    const char* name[3] = {"off", "payoff", "european"};
    long long dense_steps = 0;
    for (int m = 0; m < 3 && rc == 0; ++m) {
        rc = omc_set_option(ctx, "bounds_suboptimality", m);
        if (rc != 0) break;
        omc_bounds out;
        rc = omc_price_american_bounds(ctx, &p, &cfg, NULL, NULL, NULL, NULL, &out);
        if (rc != 0) break;
        if (m == 0) dense_steps = (long long)out.inner_path_steps;
        printf("check %s put, suboptimality %d, n_inner %lld: bounds [%.6f, %.6f]  se %.6f / %.6f  inner path-steps %lld "
               "(%.3f of the unchecked call's)  upper %.3f ms\n", name[m], m, (long long)cfg.n_inner, out.lower, out.upper,
               out.se_lower, out.se_upper, (long long)out.inner_path_steps,
               dense_steps ? (double)out.inner_path_steps / (double)dense_steps : 1.0, out.ms_upper);
    }
    if (rc != 0) {
        fprintf(stderr, "omc call failed: %d (%s)\n", rc, omc_last_error());
        omc_ctx_destroy(ctx);
        return 1;
    }
    omc_set_option(ctx, "bounds_suboptimality", 0); /* the context's defaults again */
    omc_set_option(ctx, "bounds_control_variate", 0);
    omc_ctx_destroy(ctx);
    return 0;
}
