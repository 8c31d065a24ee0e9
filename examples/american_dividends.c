/* C host for libomc.so (include/omc.h): an American call and put on a stock that pays dividends, on GPU 0 through
 * omc_price_american_div -- first with a continuous yield of 3 %, then with four quarterly cash dividends of 0.75 --
 * next to the call on the stock that pays nothing (never exercised early: the European price at LSM cost).
 *
 *   gcc -O2 -I include examples/american_dividends.c -o /tmp/american_dividends \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/american_dividends [n_paths] [n_steps] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc.h"

static int run(omc_ctx* ctx, const char* name, int is_put, double q, const omc_dividend* d, int n_div, int64_t n_paths,
               int n_steps)
{
    omc_params p;
    memset(&p, 0, sizeof p);
    p.model = OMC_MODEL_GBM;
    p.is_put = is_put;
    p.semantics = OMC_SEM_TWO_PASS;
    p.antithetic = 1;
    p.n_paths = n_paths;
    p.n_steps = n_steps;
    p.S0 = 100.0; p.K = 100.0; p.r = 0.05; p.sigma = 0.2; p.T = 1.0;
    p.seed = 42;
    omc_div_result out;
    const int rc = omc_price_american_div(ctx, &p, q, d, n_div, &out, NULL, 0);
    if (rc != 0) {
        fprintf(stderr, "omc_price_american_div (%s): %d (%s)\n", name, rc, omc_last_error());
        return 1;
    }
    printf("%s: price %.6f  exercised %lld of %lld  dividend steps %d (first %d)  folded %lld\n", name, out.base.price,
           (long long)out.base.n_exercised, (long long)out.base.n_paths, out.n_div_steps, out.first_div_step,
           (long long)out.base.folded);
    printf("%s: kernels: paths %.3f ms, total %.3f ms\n", name, out.ms_div_paths, out.base.ms_total);
    return 0;
}

int main(int argc, char** argv)
{
    const int64_t n_paths = argc > 1 ? atoll(argv[1]) : 1000000;
    const int n_steps = argc > 2 ? atoi(argv[2]) : 252;
    omc_dividend quarterly[4];
    memset(quarterly, 0, sizeof quarterly);
    for (int i = 0; i < 4; ++i) {
        quarterly[i].t = 0.25 * (i + 1) - 0.125;
        quarterly[i].amount = 0.75;
        quarterly[i].kind = OMC_DIV_CASH;
    }
    omc_ctx* ctx = NULL;
    int rc = omc_ctx_create(0, NULL, &ctx);
    if (rc != 0) {
        fprintf(stderr, "omc_ctx_create: %d (%s)\n", rc, omc_last_error());
        return 1;
    }
    rc = run(ctx, "call, no dividends", 0, 0.0, NULL, 0, n_paths, n_steps);
    if (rc == 0) rc = run(ctx, "call, yield 3 %", 0, 0.03, NULL, 0, n_paths, n_steps);
    if (rc == 0) rc = run(ctx, "call, quarterly cash 0.75", 0, 0.0, quarterly, 4, n_paths, n_steps);
    if (rc == 0) rc = run(ctx, "put, quarterly cash 0.75", 1, 0.0, quarterly, 4, n_paths, n_steps);
    omc_ctx_destroy(ctx);
    return rc;
}
