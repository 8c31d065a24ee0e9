/* C host for libomc.so (include/omc.h): a chain of American options of one expiry -- puts at K = 80 .. 115 in steps of 5
 * and calls at K = 100, 105 -- on S0 = 100, r = 0.05, sigma = 0.2, T = 1, priced on GPU 0 from ONE set of paths through
 * omc_price_american_chain (two-pass flow, 1,000,000 paths, seed 42).  Every line carries the bits of the
 * omc_price_american call for that strike and side.
 *
 *   gcc -O2 -I include examples/american_chain.c -o /tmp/american_chain \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/american_chain [n_steps] [n_paths] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc.h"

int main(int argc, char** argv)
{
    enum { N_ENTRIES = 10 };
    omc_chain_entry e[N_ENTRIES];
    memset(e, 0, sizeof e);
    for (int i = 0; i < 8; ++i) {
        e[i].K = 80.0 + 5.0 * i;
        e[i].is_put = 1;
    }
    e[8].K = 100.0;
    e[9].K = 105.0;
    omc_params p;
    memset(&p, 0, sizeof p);
    p.model = OMC_MODEL_GBM;
    p.semantics = OMC_SEM_TWO_PASS;
    p.antithetic = 1;
    p.n_steps = argc > 1 ? atoi(argv[1]) : 252;
    p.n_paths = argc > 2 ? atoll(argv[2]) : 1000000;
    p.S0 = 100.0; p.r = 0.05; p.sigma = 0.2; p.T = 1.0; /* p.K and p.is_put are ignored: the entries carry them */
    p.seed = 42;
    omc_ctx* ctx = NULL;
    int rc = omc_ctx_create(0, NULL, &ctx);
    if (rc != 0) {
        fprintf(stderr, "omc_ctx_create: %d (%s)\n", rc, omc_last_error());
        return 1;
    }
    omc_result res[N_ENTRIES];
    omc_chain_info info;
    rc = omc_price_american_chain(ctx, &p, e, N_ENTRIES, res, NULL, &info);
    if (rc != 0) {
        fprintf(stderr, "omc_price_american_chain: %d (%s)\n", rc, omc_last_error());
        omc_ctx_destroy(ctx);
        return 1;
    }
    for (int i = 0; i < N_ENTRIES; ++i)
        printf("%-4s K = %6.2f  price %.6f  std %.6f  exercised early %lld of %lld\n", e[i].is_put ? "put" : "call", e[i].K,
               res[i].price, res[i].std, (long long)res[i].n_exercised, (long long)res[i].n_paths);
    printf("%s storage, %s sweeps in %d launches per pass (width %d); kernels: paths %.3f ms, pass 1 %.3f ms, pass 2 %.3f ms, "
           "total %.3f ms\n", info.folded ? "folded" : "full", info.fused ? "fused" : "single-strike", info.n_launch_groups,
           omc_chain_width(ctx, &p, N_ENTRIES), info.ms_paths, info.ms_pass1, info.ms_pass2, info.ms_total);
    omc_ctx_destroy(ctx);
    return 0;
}
