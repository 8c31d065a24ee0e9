/* C host for libomc.so (include/omc_chain_bounds.h): Andersen-Broadie bounds for a chain of eight puts of one expiry
 * (strikes 80 .. 120 on S0 = 100, r = 0.05, sigma = 0.2, T = 1) on GPU 0 through ONE omc_price_american_chain_bounds call --
 * the fitting paths, the lower-bound paths, the outer paths and every inner path are simulated once for all eight -- and,
 * beside each, the bracket of the quote's own omc_price_american_bounds call with the same sizes, seed and streams.  The
 * lower bounds are equal bit for bit; the upper bounds differ by the order of float64 sums alone, so
 * each chain bracket holds its single-call bracket to a relative 1.2e-15.
 *
 *   gcc -O2 -I include examples/american_chain_bounds.c -o /tmp/american_chain_bounds \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/american_chain_bounds [n_steps] [n_lower] [n_outer] [n_inner] */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc_chain_bounds.h"

#define N_QUOTES 8

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
    omc_chain_entry e[N_QUOTES];
    memset(e, 0, sizeof e);
    for (int i = 0; i < N_QUOTES; ++i) {
        e[i].K = 80.0 + 40.0 * i / (N_QUOTES - 1);
        e[i].is_put = 1;
    }
    omc_ctx* ctx = NULL;
    int rc = omc_ctx_create(0, NULL, &ctx);
    if (rc != 0) {
        fprintf(stderr, "omc_ctx_create: %d (%s)\n", rc, omc_last_error());
        return 1;
    }
    omc_bounds out[N_QUOTES];
    omc_chain_bounds_info info;
    rc = omc_price_american_chain_bounds(ctx, &p, e, N_QUOTES, &cfg, NULL, NULL, NULL, NULL, out, &info);
    if (rc != 0) {
        fprintf(stderr, "omc_price_american_chain_bounds: %d (%s)\n", rc, omc_last_error());
        omc_ctx_destroy(ctx);
        return 1;
    }
    const double tol = 1.2e-15; /* 4 x the measured worst deviation of an upper bound */
    long long own_steps = 0;
    double own_ms = 0.0;
    int held = 0;
    for (int i = 0; i < N_QUOTES; ++i) {
        omc_params q = p;
        q.K = e[i].K;
        q.is_put = e[i].is_put;
        omc_bounds one;
        rc = omc_price_american_bounds(ctx, &q, &cfg, NULL, NULL, NULL, NULL, &one);
        if (rc != 0) {
            fprintf(stderr, "omc_price_american_bounds: %d (%s)\n", rc, omc_last_error());
            omc_ctx_destroy(ctx);
            return 1;
        }
        const int holds = out[i].lower <= one.lower && out[i].upper >= one.upper * (1.0 - tol) &&
                          fabs(out[i].upper - one.upper) <= tol * one.upper && out[i].inner_path_steps == one.inner_path_steps;
        held += holds;
        own_steps += one.inner_path_steps;
        own_ms += one.ms_total;
        printf("put K = %7.3f  chain [%.6f, %.6f]  se %.6f / %.6f  single [%.6f, %.6f]  holds it: %s\n", e[i].K, out[i].lower,
               out[i].upper, out[i].se_lower, out[i].se_upper, one.lower, one.upper, holds ? "yes" : "NO");
    }
    printf("%d of %d chain brackets hold their single-call bracket\n", held, N_QUOTES);
    printf("inner path-steps: %lld simulated by the chain in %d group(s), %lld by the single calls together\n",
           (long long)info.inner_path_steps_simulated, (int)info.n_groups, own_steps);
    printf("kernels: chain fit %.3f ms, lower %.3f ms, upper %.3f ms, total %.3f ms; the single calls together %.3f ms\n",
           info.ms_fit, info.ms_lower, info.ms_upper, info.ms_total, own_ms);
    omc_ctx_destroy(ctx);
    return held == N_QUOTES ? 0 : 2;
}
