/* C host for libomc.so (include/omc.h): the American price of the BASELINE config-2 option on GPU 0 and its five Greeks
 * (frozen-policy pathwise Greeks of the two-pass flow, omc_price_american_greeks).
 *
 *   gcc -O2 -I include examples/american_greeks.c -o /tmp/american_greeks \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/american_greeks [n_paths] [n_steps] [bump]
 *
 * Raw units: delta per unit S0, gamma per unit S0^2, vega per unit sigma, rho per unit r, theta = -dV/dT per year. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc.h"

int main(int argc, char** argv)
{
    omc_ctx* ctx = NULL;
    int rc = omc_ctx_create(0, NULL, &ctx);
    if (rc != 0) {
        fprintf(stderr, "omc_ctx_create: %d (%s)\n", rc, omc_last_error());
        return 1;
    }
    omc_params p;
    memset(&p, 0, sizeof p);
    p.model = OMC_MODEL_GBM;
    p.is_put = 1;
    p.semantics = OMC_SEM_TWO_PASS;
    p.antithetic = 1;
    p.n_paths = argc > 1 ? atoll(argv[1]) : 1000000;
    p.n_steps = argc > 2 ? atoi(argv[2]) : 252;
    p.S0 = 100.0; p.K = 100.0; p.r = 0.05; p.sigma = 0.2; p.T = 1.0;
    p.seed = 42;
    const double bump = argc > 3 ? atof(argv[3]) : 0.01;
    omc_greeks g;
    rc = omc_price_american_greeks(ctx, &p, bump, NULL, NULL, &g);
    if (rc != 0) {
        fprintf(stderr, "omc_price_american_greeks: %d (%s)\n", rc, omc_last_error());
        omc_ctx_destroy(ctx);
        return 1;
    }
    printf("price %.6f  paths %lld  exercised %lld  storage: %s\n", g.base.price, (long long)g.base.n_paths,
           (long long)g.base.n_exercised, g.base.folded ? "antithetic-folded" : "full");
    printf("delta %.6f  se %.6f\n", g.delta, g.se_delta);
    printf("gamma %.6f  se %.6f\n", g.gamma, g.se_gamma);
    printf("vega %.6f  se %.6f\n", g.vega, g.se_vega);
    printf("rho %.6f  se %.6f\n", g.rho, g.se_rho);
    printf("theta %.6f  se %.6f\n", g.theta, g.se_theta);
    printf("kernels: paths %.3f ms, pass 1 %.3f ms, greeks sweep %.3f ms\n", g.base.ms_paths, g.base.ms_pass1, g.ms_greeks);
    omc_ctx_destroy(ctx);
    return 0;
}
