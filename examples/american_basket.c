/* C host for libomc.so (include/omc.h): American options on several correlated GBM assets, on GPU 0 through
 * omc_price_american_basket -- a 3-asset arithmetic basket put, a 2-asset best-of call, and a 1-asset basket, which is
 * the single-stock put with a dividend yield.  The exercise policy is a function of the index alone.
 *
 *   gcc -O2 -I include examples/american_basket.c -o /tmp/american_basket \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/american_basket [n_paths] [n_steps] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc.h"

static int run(omc_ctx* ctx, const char* name, const omc_basket* b, int is_put, int64_t n_paths, int n_steps)
{
    omc_params p;
    memset(&p, 0, sizeof p);
    p.model = OMC_MODEL_GBM;
    p.is_put = is_put;
    p.semantics = OMC_SEM_TWO_PASS;
    p.antithetic = 1;
    p.n_paths = n_paths;
    p.n_steps = n_steps;
    p.K = 100.0; p.r = 0.05; p.T = 1.0; /* S0 and sigma are not read: the basket carries them */
    p.seed = 42;
    double geo[3];
    omc_basket_result out;
    int rc = omc_basket_table(&p, b, NULL, NULL, NULL, NULL, geo); /* host only: the argument checks and the constants */
    if (rc == 0) rc = omc_price_american_basket(ctx, &p, b, &out, NULL, NULL, 0);
    if (rc != 0) {
        fprintf(stderr, "omc_price_american_basket (%s): %d (%s)\n", name, rc, omc_last_error());
        return 1;
    }
    printf("%s: price %.6f  exercised %lld of %lld  index0 %.6f  assets %d  sigma_G %.6f  paths %.3f ms  total %.3f ms\n", name,
           out.base.price, (long long)out.base.n_exercised, (long long)out.base.n_paths, out.index0, (int)out.n_assets, geo[1],
           out.ms_basket_paths, out.base.ms_total);
    return 0;
}

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
    omc_basket b3, b2, b1;
    memset(&b3, 0, sizeof b3);
    b3.n_assets = 3; b3.kind = OMC_BASKET_ARITHMETIC;
    const double rho3[9] = {1.0, 0.5, 0.2, 0.5, 1.0, -0.3, 0.2, -0.3, 1.0};
    const double s3[3] = {100.0, 95.0, 105.0}, v3[3] = {0.2, 0.25, 0.3}, q3[3] = {0.01, 0.0, 0.03}, w3[3] = {0.5, 0.3, 0.2};
    for (int i = 0; i < 3; ++i) { b3.S0[i] = s3[i]; b3.sigma[i] = v3[i]; b3.q[i] = q3[i]; b3.w[i] = w3[i]; }
    memcpy(b3.rho, rho3, sizeof rho3);
    memset(&b2, 0, sizeof b2);
    b2.n_assets = 2; b2.kind = OMC_BASKET_BEST_OF;
    const double rho2[4] = {1.0, 0.6, 0.6, 1.0};
    b2.S0[0] = 100.0; b2.S0[1] = 95.0; b2.sigma[0] = 0.2; b2.sigma[1] = 0.3; b2.q[0] = 0.02; b2.q[1] = 0.04;
    b2.w[0] = b2.w[1] = 1.0;
    memcpy(b2.rho, rho2, sizeof rho2);
    memset(&b1, 0, sizeof b1);
    b1.n_assets = 1; b1.kind = OMC_BASKET_ARITHMETIC;
    b1.S0[0] = 100.0; b1.sigma[0] = 0.2; b1.q[0] = 0.02; b1.w[0] = 1.0; b1.rho[0] = 1.0;
    rc = run(ctx, "basket put, 3 assets", &b3, 1, n_paths, n_steps);
    if (rc == 0) rc = run(ctx, "best-of call, 2 assets", &b2, 0, n_paths, n_steps);
    if (rc == 0) rc = run(ctx, "basket put, 1 asset", &b1, 1, n_paths, n_steps);
    omc_ctx_destroy(ctx);
    return rc;
}
