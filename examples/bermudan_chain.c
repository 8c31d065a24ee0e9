/* C host for libomc.so (include/omc.h): ONE strike as four entries of one chain -- the American put (exercise on every
 * date of a daily grid), the monthly and the quarterly Bermudan put (omc_chain_entry::exercise_every = 21 and 63: every
 * 21st / 63rd date counted back from expiry) and the European value of the flow (exercise_every = n_steps: no early date)
 * -- on S0 = 100, K = 100, r = 0.05, sigma = 0.2, T = 1, priced on GPU 0 from ONE set of paths through
 * omc_price_american_chain (two-pass flow, 252 dates, 1,000,000 paths, seed 42).  The four values share their paths, so
 * the early-exercise premia below carry no Monte-Carlo noise of their own.
 *
 *   gcc -O2 -I include examples/bermudan_chain.c -o /tmp/bermudan_chain \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/bermudan_chain [n_steps] [n_paths] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc.h"

int main(int argc, char** argv)
{
    enum { N_ENTRIES = 4 };
    static const char* const name[N_ENTRIES] = {"american", "monthly", "quarterly", "european"};
    omc_params p;
    memset(&p, 0, sizeof p);
    p.model = OMC_MODEL_GBM;
    p.semantics = OMC_SEM_TWO_PASS;
    p.antithetic = 1;
    p.n_steps = argc > 1 ? atoi(argv[1]) : 252;
    p.n_paths = argc > 2 ? atoll(argv[2]) : 1000000;
    p.S0 = 100.0; p.r = 0.05; p.sigma = 0.2; p.T = 1.0; /* p.K and p.is_put are ignored: the entries carry them */
    p.seed = 42;
    omc_chain_entry e[N_ENTRIES];
    memset(e, 0, sizeof e);
    for (int i = 0; i < N_ENTRIES; ++i) {
        e[i].K = 100.0;
        e[i].is_put = 1;
    }
    e[0].exercise_every = 0; /* every date */
    e[1].exercise_every = 21;
    e[2].exercise_every = 63;
    e[3].exercise_every = p.n_steps;
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
    for (int i = 0; i < N_ENTRIES; ++i) {
        const int k = e[i].exercise_every;
        const int dates = k >= 2 ? (p.n_steps - 1) / k : p.n_steps - 1;
        printf("%-9s every %3d  early dates %3d  price %.6f  premium over european %.6f  exercised early %lld of %lld\n", name[i],
               k, dates, res[i].price, res[i].price - res[3].price, (long long)res[i].n_exercised, (long long)res[i].n_paths);
    }
    printf("%s storage, %s sweeps; kernels: paths %.3f ms, pass 1 %.3f ms, pass 2 %.3f ms, total %.3f ms\n",
           info.folded ? "folded" : "full", info.fused ? "fused" : "single-strike", info.ms_paths, info.ms_pass1, info.ms_pass2,
           info.ms_total);
    omc_ctx_destroy(ctx);
    return 0;
}
