/* C host for libomc.so (include/omc.h): Asian (average-price) options with early exercise on one GBM stock -- S0 = 100,
 * K = 100, r = 5 %, sigma = 30 %, T = 1, the average taken over the exercise dates 1 .. t of the grid.  The Asian payoffs are
 * index kinds of the multi-asset entry points (OMC_BASKET_ASIAN_ARITHMETIC / _GEOMETRIC; one asset of weight 1 is the plain
 * Asian option):
 *   omc_price_american_basket                   the two-pass price of the arithmetic and of the geometric average put;
 *   omc_price_american_basket_bounds            Andersen-Broadie bounds, the policy regresses on the average alone;
 *   omc_price_american_basket_bounds_runnerup   ... on the average and the spot: the Markov state of the option is the pair.
 * The Greeks entry point refuses these kinds (-32).
 *
 *   gcc -O2 -I include examples/american_asian.c -o /tmp/american_asian \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/american_asian [n_paths] [n_steps] [n_lower] [n_outer] [n_inner] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc.h"

static void print_bounds(const char* name, const omc_basket_bounds* out)
{
    const omc_bounds* o = &out->bounds;
    printf("%-16s: bounds [%.6f, %.6f]  se %.6f / %.6f  95%% interval [%.6f, %.6f]\n", name, o->lower, o->upper, o->se_lower,
           o->se_upper, o->ci_lo, o->ci_hi);
    printf("%-16s  %lld lower paths stopped before maturity, inner path-steps %lld; kernels: fit %.3f ms, lower %.3f ms, "
           "upper %.3f ms, total %.3f ms\n", "", (long long)o->n_exercised_lower, (long long)o->inner_path_steps, o->ms_fit,
           o->ms_lower, o->ms_upper, o->ms_total);
}

int main(int argc, char** argv)
{
    omc_params p;
    memset(&p, 0, sizeof p);
    p.model = OMC_MODEL_GBM;
    p.is_put = 1;
    p.semantics = OMC_SEM_TWO_PASS;
    p.antithetic = 1;
    p.n_paths = argc > 1 ? atoll(argv[1]) : 1000000;
    p.n_steps = argc > 2 ? atoi(argv[2]) : 12;
    p.S0 = 100.0; p.sigma = 0.3; /* not read: the asset is in the basket */
    p.K = 100.0; p.r = 0.05; p.T = 1.0;
    p.seed = 42;
    omc_bounds_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.policy = OMC_SEM_TEXTBOOK;
    cfg.n_lower = argc > 3 ? atoll(argv[3]) : 1000000;
    cfg.n_outer = argc > 4 ? atoll(argv[4]) : 4096;
    cfg.n_inner = argc > 5 ? atoll(argv[5]) : 512;
    cfg.stream_lower = 1;
    cfg.stream_outer = 2;
    cfg.stream_inner = 3;
    omc_basket b;
    memset(&b, 0, sizeof b);
    b.n_assets = 1;
    b.S0[0] = 100.0; b.sigma[0] = 0.3; b.q[0] = 0.0; b.w[0] = 1.0;
    b.rho[0] = 1.0;
    omc_ctx* ctx = NULL;
    int rc = omc_ctx_create(0, NULL, &ctx);
    if (rc != 0) {
        fprintf(stderr, "omc_ctx_create: %d (%s)\n", rc, omc_last_error());
        return 1;
    }
    const int kinds[2] = {OMC_BASKET_ASIAN_ARITHMETIC, OMC_BASKET_ASIAN_GEOMETRIC};
    const char* names[2] = {"arithmetic", "geometric"};
    for (int i = 0; i < 2; ++i) {
        omc_basket_result out;
        b.kind = kinds[i];
        rc = omc_price_american_basket(ctx, &p, &b, &out, NULL, NULL, 0);
        if (rc != 0) {
            fprintf(stderr, "omc_price_american_basket: %d (%s)\n", rc, omc_last_error());
            omc_ctx_destroy(ctx);
            return 1;
        }
        printf("%s average put: price %.6f  (%lld paths, %d dates, %lld exercised early; paths %.3f ms, total %.3f ms)\n",
               names[i], out.base.price, (long long)out.base.n_paths, p.n_steps, (long long)out.base.n_exercised,
               out.ms_basket_paths, out.base.ms_total);
    }
    b.kind = OMC_BASKET_ASIAN_ARITHMETIC;
    omc_basket_bounds average, both;
    rc = omc_price_american_basket_bounds(ctx, &p, &b, &cfg, NULL, NULL, NULL, NULL, &average);
    if (rc == 0) rc = omc_price_american_basket_bounds_runnerup(ctx, &p, &b, &cfg, NULL, NULL, NULL, NULL, &both);
    if (rc != 0) {
        fprintf(stderr, "price bounds: %d (%s)\n", rc, omc_last_error());
        omc_ctx_destroy(ctx);
        return 1;
    }
    printf("arithmetic average put, Bermudan game on the grid; the policy regresses on the\n");
    print_bounds("average alone", &average);
    print_bounds("average and spot", &both);
    printf("lower bound: %+.6f with the spot (%.1f standard errors)\n", both.bounds.lower - average.bounds.lower,
           (both.bounds.lower - average.bounds.lower) / (average.bounds.se_lower > 0.0 ? average.bounds.se_lower : 1.0));
    omc_basket_greeks g;
    rc = omc_price_american_basket_greeks(ctx, &p, &b, 0.01, 0, NULL, NULL, &g);
    printf("Greeks: %s (%d)\n", rc == 0 ? "computed" : "refused", rc);
    omc_ctx_destroy(ctx);
    return 0;
}
