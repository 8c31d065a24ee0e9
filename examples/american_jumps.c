/* C host for libomc.so (include/omc.h): an American put under jump-diffusion, on GPU 0 through
 * omc_price_american_jump -- Merton's model (jumps on GBM), then Bates's (jumps on Heston) -- next to the put without
 * jumps, which the same entry point prices with lambda = 0.
 *
 *   gcc -O2 -I include examples/american_jumps.c -o /tmp/american_jumps \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/american_jumps [n_paths] [n_steps] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc.h"

static int run(omc_ctx* ctx, const char* name, int model, double lambda, int64_t n_paths, int n_steps)
{
    omc_params p;
    memset(&p, 0, sizeof p);
    p.model = model;
    p.is_put = 1;
    p.semantics = OMC_SEM_TWO_PASS;
    p.antithetic = 1;
    p.n_paths = n_paths;
    p.n_steps = n_steps;
    p.S0 = 100.0; p.K = 100.0; p.r = 0.05; p.sigma = 0.2; p.T = 1.0;
    p.v0 = 0.04; p.kappa = 2.0; p.theta = 0.04; p.xi = 0.3; p.rho = -0.7;
    p.seed = 42;
    omc_jump j;
    j.lambda = lambda; j.mu_j = -0.1; j.sigma_j = 0.15;
    uint32_t thr[16];
    omc_jump_result out;
    int rc = omc_jump_table(&p, &j, 0.02, thr, NULL, NULL);  /* host only: the argument checks and the Poisson table */
    if (rc == 0) rc = omc_price_american_jump(ctx, &p, &j, 0.02, &out, NULL, 0);
    if (rc != 0) {
        fprintf(stderr, "omc_price_american_jump (%s): %d (%s)\n", name, rc, omc_last_error());
        return 1;
    }
    printf("%s: price %.6f  exercised %lld of %lld  kappa %.6f  drift rate %.6f  P(no jump in a step) %.6f  folded %lld\n",
           name, out.base.price, (long long)out.base.n_exercised, (long long)out.base.n_paths, out.kappa, out.drift_rate,
           thr[0] / 16777216.0, (long long)out.base.folded);
    printf("%s: kernels: paths %.3f ms, total %.3f ms\n", name, out.ms_jump_paths, out.base.ms_total);
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
    rc = run(ctx, "merton, lambda 1", OMC_MODEL_GBM, 1.0, n_paths, n_steps);
    if (rc == 0) rc = run(ctx, "bates, lambda 1", OMC_MODEL_HESTON, 1.0, n_paths, n_steps);
    if (rc == 0) rc = run(ctx, "gbm, no jumps", OMC_MODEL_GBM, 0.0, n_paths, n_steps);
    omc_ctx_destroy(ctx);
    return rc;
}
