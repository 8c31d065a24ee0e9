/* C host for libomc.so (include/omc.h): the ATM American put under the Heston model (S0 = K = 100, r = 0.05, T = 1;
 * v0 = theta = 0.04, kappa = 2, xi = 0.3, rho = -0.7) on GPU 0 with Andersen's quadratic-exponential scheme
 * (heston_scheme = OMC_HESTON_QE; the rule is written out in include/omc.h), next to the same pricing with the
 * full-truncation Euler scheme on the same Philox stream.  Two-pass flow, 100,000 paths, seed 42.
 * OMC_HESTON_QE needs kappa, theta and xi positive: the call returns -36 otherwise and launches nothing.
 *
 *   gcc -O2 -I include examples/american_heston_qe.c -o /tmp/american_heston_qe \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/american_heston_qe [n_steps] [n_paths] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc.h"

int main(int argc, char** argv)
{
    omc_params p;
    memset(&p, 0, sizeof p);
    p.model = OMC_MODEL_HESTON;
    p.is_put = 1;
    p.semantics = OMC_SEM_TWO_PASS;
    p.antithetic = 1;
    p.n_steps = argc > 1 ? atoi(argv[1]) : 50;
    p.n_paths = argc > 2 ? atoll(argv[2]) : 100000;
    p.S0 = 100.0; p.K = 100.0; p.r = 0.05; p.T = 1.0;
    p.v0 = 0.04; p.kappa = 2.0; p.theta = 0.04; p.xi = 0.3; p.rho = -0.7;
    p.seed = 42;
    omc_ctx* ctx = NULL;
    int rc = omc_ctx_create(0, NULL, &ctx);
    if (rc != 0) {
        fprintf(stderr, "omc_ctx_create: %d (%s)\n", rc, omc_last_error());
        return 1;
    }
    const int schemes[2] = {OMC_HESTON_QE, OMC_HESTON_FULL_TRUNCATION};
    const char* names[2] = {"qe", "full truncation"};
    for (int k = 0; k < 2; ++k) {
        omc_result res;
        p.heston_scheme = schemes[k];
        rc = omc_price_american(ctx, &p, &res, NULL, 0);
        if (rc != 0) {
            fprintf(stderr, "omc_price_american (%s): %d (%s)\n", names[k], rc, omc_last_error());
            omc_ctx_destroy(ctx);
            return 1;
        }
        printf("american heston put, %s: price %.6f  (%lld paths, %d steps, %lld exercised early; paths %.3f ms, lsm %.3f ms)\n",
               names[k], res.price, (long long)res.n_paths, p.n_steps, (long long)res.n_exercised, res.ms_paths, res.ms_lsm);
    }
    p.heston_scheme = OMC_HESTON_QE;
    p.xi = 0.0;
    omc_result res;
    rc = omc_price_american(ctx, &p, &res, NULL, 0);
    printf("xi = 0 under qe: %d (%s)\n", rc, omc_last_error());
    omc_ctx_destroy(ctx);
    return rc == -36 ? 0 : 1;
}
