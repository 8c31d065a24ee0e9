/* C host for libomc.so (include/omc.h): the frozen-policy pathwise Greeks of an American put on an arithmetic basket of
 * three correlated GBM assets, on GPU 0 through omc_price_american_basket_greeks -- per asset delta, diagonal gamma and
 * vega (the hedge of the basket), and rho and theta of the option.
 *
 *   gcc -O2 -I include examples/american_basket_greeks.c -o /tmp/american_basket_greeks \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/american_basket_greeks [n_paths] [n_steps] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc.h"

int main(int argc, char** argv)
{
    const int64_t n_paths = argc > 1 ? atoll(argv[1]) : 1000000;
    const int n_steps = argc > 2 ? atoi(argv[2]) : 252;
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
    p.n_paths = n_paths;
    p.n_steps = n_steps;
    p.K = 100.0; p.r = 0.05; p.T = 1.0; /* S0 and sigma are not read: the basket carries them */
    p.seed = 42;
    omc_basket b;
    memset(&b, 0, sizeof b);
    b.n_assets = 3; b.kind = OMC_BASKET_ARITHMETIC;
    const double rho[9] = {1.0, 0.5, 0.2, 0.5, 1.0, -0.3, 0.2, -0.3, 1.0};
    const double s[3] = {100.0, 95.0, 105.0}, v[3] = {0.2, 0.25, 0.3}, q[3] = {0.01, 0.0, 0.03}, w[3] = {0.5, 0.3, 0.2};
    for (int i = 0; i < 3; ++i) { b.S0[i] = s[i]; b.sigma[i] = v[i]; b.q[i] = q[i]; b.w[i] = w[i]; }
    memcpy(b.rho, rho, sizeof rho);
    omc_basket_greeks g;
    rc = omc_price_american_basket_greeks(ctx, &p, &b, 0.01, 1, NULL, NULL, &g);
    if (rc != 0) {
        fprintf(stderr, "omc_price_american_basket_greeks: %d (%s)\n", rc, omc_last_error());
        omc_ctx_destroy(ctx);
        return 1;
    }
    printf("basket put, 3 assets: price %.6f  exercised %lld of %lld  index0 %.6f\n", g.base.base.price,
           (long long)g.base.base.n_exercised, (long long)g.base.base.n_paths, g.base.index0);
    for (int i = 0; i < g.base.n_assets; ++i)
        printf("asset %d: delta %.8e (se %.2e)  gamma %.8e (se %.2e)  vega %.8e (se %.2e)  price at S0 (1 +- %.2f): %.6f / %.6f\n",
               i, g.delta[i], g.se_delta[i], g.gamma[i], g.se_gamma[i], g.vega[i], g.se_vega[i], g.bump, g.price_up[i],
               g.price_down[i]);
    printf("rho %.8e (se %.2e)  theta %.8e (se %.2e)\n", g.rho, g.se_rho, g.theta, g.se_theta);
    printf("paths %.3f ms  pass 1 %.3f ms  Greeks sweep %.3f ms\n", g.base.ms_basket_paths, g.base.base.ms_pass1, g.ms_greeks);
    omc_ctx_destroy(ctx);
    return 0;
}
