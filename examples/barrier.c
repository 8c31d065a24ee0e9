/* C host for libomc.so (include/omc.h): two barrier options on GPU 0 through omc_price_barrier --
 * a down-and-out American put (H = 90, discrete monitoring, two-pass LSM on the encoded path matrix) and a
 * European up-and-in call (H = 120, continuous monitoring).
 *
 *   gcc -O2 -I include examples/barrier.c -o /tmp/barrier \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/barrier [n_paths] [n_steps] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc.h"

static int run(omc_ctx* ctx, const char* name, int is_put, int kind, int monitoring, int american, double H,
               int64_t n_paths, int n_steps)
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
    omc_barrier b;
    memset(&b, 0, sizeof b);
    b.kind = kind;
    b.monitoring = monitoring;
    b.american = american;
    b.H = H;
    omc_barrier_result out;
    const int rc = omc_price_barrier(ctx, &p, &b, &out, NULL, 0);
    if (rc != 0) {
        fprintf(stderr, "omc_price_barrier (%s): %d (%s)\n", name, rc, omc_last_error());
        return 1;
    }
    printf("%s: price %.6f  exercised %lld  hit_prob %.6f\n", name, out.base.price, (long long)out.base.n_exercised,
           out.hit_prob);
    printf("%s: euro_out %.6f se %.6f  euro_in %.6f se %.6f\n", name, out.euro_out, out.euro_out_se, out.euro_in,
           out.euro_in_se);
    printf("%s: kernels: barrier paths %.3f ms, total %.3f ms\n", name, out.ms_barrier_paths, out.base.ms_total);
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
    rc = run(ctx, "down-and-out american put", 1, OMC_BARRIER_DOWN_OUT, OMC_MONITOR_DISCRETE, 1, 90.0, n_paths, n_steps);
    if (rc == 0)
        rc = run(ctx, "up-and-in european call", 0, OMC_BARRIER_UP_IN, OMC_MONITOR_CONTINUOUS, 0, 120.0, n_paths, n_steps);
    omc_ctx_destroy(ctx);
    return rc;
}
