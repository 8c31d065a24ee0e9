/* C host for libomc.so (include/omc.h): what the exercise policy sees, on the two-asset max-call benchmark of
 * Broadie-Glasserman / Andersen-Broadie (2004) -- a best-of call on two independent GBM assets, S0 = 100 each (or argv[1]),
 * K = 100, r = 5 %, yield 10 %, sigma = 20 %, T = 3, nine exercise dates; published value at S0 = 90 / 100 / 110: 8.075 /
 * 13.902 / 21.345.  Both brackets come from textbook Longstaff-Schwartz fits on 100,000 paths (seed 42, stream 0; lower /
 * outer / inner paths on streams 1 / 2 / 3):
 *   omc_price_american_basket_bounds            regresses on the index max(S_1, S_2) alone;
 *   omc_price_american_basket_bounds_runnerup   on the index and the runner-up, here min(S_1, S_2).
 * The lower bound is what the policy earns on fresh paths, so the second one sits closer to the value.
 *
 *   gcc -O2 -I include examples/american_basket_runnerup_bounds.c -o /tmp/american_basket_runnerup_bounds \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/american_basket_runnerup_bounds [S0] [n_lower] [n_outer] [n_inner] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc.h"

static void print_bounds(const char* name, const omc_basket_bounds* out)
{
    const omc_bounds* o = &out->bounds;
    printf("%-17s: bounds [%.6f, %.6f]  se %.6f / %.6f  95%% interval [%.6f, %.6f]\n", name, o->lower, o->upper, o->se_lower,
           o->se_upper, o->ci_lo, o->ci_hi);
    printf("%-17s  %lld lower paths stopped before maturity, inner path-steps %lld; kernels: fit %.3f ms, lower %.3f ms, "
           "upper %.3f ms, total %.3f ms\n", "", (long long)o->n_exercised_lower, (long long)o->inner_path_steps, o->ms_fit,
           o->ms_lower, o->ms_upper, o->ms_total);
}

int main(int argc, char** argv)
{
    const double S0 = argc > 1 ? atof(argv[1]) : 100.0;
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
    p.is_put = 0;
    p.semantics = OMC_SEM_TWO_PASS; /* what the multi-asset entry points ask for; cfg.policy chooses the fits */
    p.antithetic = 1;
    p.n_paths = 100000;
    p.n_steps = 9;
    p.S0 = S0; p.sigma = 0.2; /* not read: the assets are in the basket */
    p.K = 100.0; p.r = 0.05; p.T = 3.0;
    p.seed = 42;
    omc_basket b;
    memset(&b, 0, sizeof b);
    b.n_assets = 2;
    b.kind = OMC_BASKET_BEST_OF;
    for (int i = 0; i < 2; ++i) {
        b.S0[i] = S0; b.sigma[i] = 0.2; b.q[i] = 0.1; b.w[i] = 1.0;
        b.rho[i * 2 + i] = 1.0;
    }
    omc_ctx* ctx = NULL;
    int rc = omc_ctx_create(0, NULL, &ctx);
    if (rc != 0) {
        fprintf(stderr, "omc_ctx_create: %d (%s)\n", rc, omc_last_error());
        return 1;
    }
    omc_basket_bounds index_only, runner_up;
    rc = omc_price_american_basket_bounds(ctx, &p, &b, &cfg, NULL, NULL, NULL, NULL, &index_only);
    if (rc == 0) rc = omc_price_american_basket_bounds_runnerup(ctx, &p, &b, &cfg, NULL, NULL, NULL, NULL, &runner_up);
    if (rc != 0) {
        fprintf(stderr, "price bounds: %d (%s)\n", rc, omc_last_error());
        omc_ctx_destroy(ctx);
        return 1;
    }
    printf("max-call on %d assets, S0 = %g, %d dates; the policy regresses on\n", (int)runner_up.n_assets, runner_up.index0,
           p.n_steps);
    print_bounds("index", &index_only);
    print_bounds("index + runner-up", &runner_up);
    printf("lower bound: %+.6f with the runner-up (%.1f standard errors)\n", runner_up.bounds.lower - index_only.bounds.lower,
           (runner_up.bounds.lower - index_only.bounds.lower) /
               (index_only.bounds.se_lower > 0.0 ? index_only.bounds.se_lower : 1.0));
    omc_ctx_destroy(ctx);
    return 0;
}
