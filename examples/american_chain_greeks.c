/* C host for libomc.so (include/omc_chain_greeks.h): a strike ladder hedged on three exercise schedules.  Every strike of
 * K = 90, 95, 100, 105, 110 is three entries of ONE chain -- the American put (exercise on every date of a daily grid), the
 * monthly Bermudan put (omc_chain_entry::exercise_every = 21) and the European value of the flow (exercise_every = n_steps)
 * -- on S0 = 100, r = 0.05, sigma = 0.2, T = 1, and omc_price_american_chain_greeks returns the frozen-policy pathwise
 * Greeks of all fifteen from ONE set of paths on GPU 0 (two-pass flow, 252 dates, 1,000,000 paths, seed 42).  The entries
 * share their paths, so the delta and vega differences between schedules below carry no Monte-Carlo noise of their own.
 *
 *   gcc -O2 -I include examples/american_chain_greeks.c -o /tmp/american_chain_greeks \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/american_chain_greeks [n_steps] [n_paths] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc_chain_greeks.h"

int main(int argc, char** argv)
{
    enum { N_STRIKES = 5, N_SCHEDULES = 3, N_ENTRIES = N_STRIKES * N_SCHEDULES };
    static const char* const name[N_SCHEDULES] = {"american", "monthly", "european"};
    omc_params p;
    memset(&p, 0, sizeof p);
    p.model = OMC_MODEL_GBM;
    p.semantics = OMC_SEM_TWO_PASS;
    p.antithetic = 1;
    p.n_steps = argc > 1 ? atoi(argv[1]) : 252;
    p.n_paths = argc > 2 ? atoll(argv[2]) : 1000000;
    p.S0 = 100.0; p.r = 0.05; p.sigma = 0.2; p.T = 1.0; /* p.K and p.is_put are ignored: the entries carry them */
    p.seed = 42;
    const int every[N_SCHEDULES] = {0, 21, p.n_steps};
    omc_chain_entry e[N_ENTRIES];
    memset(e, 0, sizeof e);
    for (int i = 0; i < N_ENTRIES; ++i) {
        e[i].K = 90.0 + 5.0 * (i / N_SCHEDULES);
        e[i].is_put = 1;
        e[i].exercise_every = every[i % N_SCHEDULES];
    }
    omc_ctx* ctx = NULL;
    int rc = omc_ctx_create(0, NULL, &ctx);
    if (rc != 0) {
        fprintf(stderr, "omc_ctx_create: %d (%s)\n", rc, omc_last_error());
        return 1;
    }
    omc_greeks g[N_ENTRIES];
    omc_chain_greeks_info info;
    rc = omc_price_american_chain_greeks(ctx, &p, e, N_ENTRIES, 0.01, NULL, NULL, g, &info);
    if (rc != 0) {
        fprintf(stderr, "omc_price_american_chain_greeks: %d (%s)\n", rc, omc_last_error());
        omc_ctx_destroy(ctx);
        return 1;
    }
    for (int i = 0; i < N_ENTRIES; ++i) {
        const omc_greeks* eu = &g[i / N_SCHEDULES * N_SCHEDULES + N_SCHEDULES - 1]; /* the strike's European entry */
        printf("K %5.1f %-8s price %.6f  delta %.6f  gamma %.6f  vega %.6f  delta - european %.6f  vega - european %.6f\n", e[i].K,
               name[i % N_SCHEDULES], g[i].base.price, g[i].delta, g[i].gamma, g[i].vega, g[i].delta - eu->delta,
               g[i].vega - eu->vega);
    }
    printf("%s storage, %d groups, %d Greeks sweep launches; kernels: paths %.3f ms, pass 1 %.3f ms, greeks %.3f ms, total %.3f ms\n",
           info.folded ? "folded" : "full", (int)info.n_groups, (int)info.n_sweep_launches, info.ms_paths, info.ms_pass1,
           info.ms_greeks, info.ms_total);
    omc_ctx_destroy(ctx);
    return 0;
}
