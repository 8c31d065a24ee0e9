/* C host for libomc.so (include/omc.h): Andersen-Broadie bounds on the Bermudan value of the ATM put under the Heston
 * model (S0 = K = 100, r = 0.05, T = 1; v0 = theta = 0.04, kappa = 2, xi = 0.3, rho = -0.7) on GPU 0 through
 * omc_price_american_bounds_heston, twice from the same Philox streams: with the textbook Longstaff-Schwartz policy on the
 * spot alone (cfg.regressors = OMC_HESTON_REG_SPOT) and with the policy on the spot and the variance state
 * (OMC_HESTON_REG_SPOT_VARIANCE), both fitted on 100,000 paths (seed 42, stream 0; lower / outer / inner paths on streams
 * 1 / 2 / 3).  The lower bounds are what either policy earns in the discretised scheme's game; either upper bound holds
 * against every policy.
 *
 *   gcc -O2 -I include examples/american_heston_sv_bounds.c -o /tmp/american_heston_sv_bounds \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/american_heston_sv_bounds [n_steps] [n_lower] [n_outer] [n_inner] [scheme: 0 reference, 1 full truncation] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc.h"

int main(int argc, char** argv)
{
    const int n_steps = argc > 1 ? atoi(argv[1]) : 50;
    static const char* const names[2] = {"spot", "spot+variance"};
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
    p.model = OMC_MODEL_HESTON;
    p.heston_scheme = argc > 5 ? atoi(argv[5]) : OMC_HESTON_REFERENCE_CLAMP;
    p.is_put = 1;
    p.semantics = OMC_SEM_TWO_PASS; /* not used by the bounds: cfg.policy chooses the fit */
    p.antithetic = 1;
    p.n_paths = 100000;
    p.n_steps = n_steps;
    p.S0 = 100.0; p.K = 100.0; p.r = 0.05; p.T = 1.0;
    p.v0 = 0.04; p.kappa = 2.0; p.theta = 0.04; p.xi = 0.3; p.rho = -0.7;
    p.seed = 42;
    omc_ctx* ctx = NULL;
    int rc = omc_ctx_create(0, NULL, &ctx);
    if (rc != 0) {
        fprintf(stderr, "omc_ctx_create: %d (%s)\n", rc, omc_last_error());
        return 1;
    }
    for (int reg = OMC_HESTON_REG_SPOT; reg <= OMC_HESTON_REG_SPOT_VARIANCE; ++reg) {
        omc_bounds out;
        cfg.regressors = reg;
        rc = omc_price_american_bounds_heston(ctx, &p, &cfg, NULL, NULL, NULL, NULL, &out);
        if (rc != 0) {
            fprintf(stderr, "omc_price_american_bounds_heston (%s): %d (%s)\n", names[reg], rc, omc_last_error());
            omc_ctx_destroy(ctx);
            return 1;
        }
        printf("policy on %s, %d dates: bounds [%.6f, %.6f]  se %.6f / %.6f  95%% interval [%.6f, %.6f]\n", names[reg],
               n_steps, out.lower, out.upper, out.se_lower, out.se_upper, out.ci_lo, out.ci_hi);
        printf("  lower: %lld paths, %lld stopped before maturity; upper: %lld outer x %lld inner, inner path-steps %lld\n",
               (long long)out.n_lower, (long long)out.n_exercised_lower, (long long)out.n_outer, (long long)out.n_inner,
               (long long)out.inner_path_steps);
        printf("  kernels: fit %.3f ms, lower %.3f ms, upper %.3f ms, total %.3f ms\n", out.ms_fit, out.ms_lower, out.ms_upper,
               out.ms_total);
    }
    omc_ctx_destroy(ctx);
    return 0;
}
