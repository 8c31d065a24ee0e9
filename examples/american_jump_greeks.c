/* C host for libomc.so (include/omc_jump_greeks.h): the hedge ratios of an ATM American put under jump-diffusion
 * (S0 = K = 100, r = 0.05, T = 1; lambda = 1 jump a year, J ~ N(-0.1, 0.15^2)) on GPU 0 through
 * omc_price_american_jump_greeks, beside the quote of omc_price_american_jump they belong to.  The exercise policy pass 1
 * fits is held fixed; one forward sweep regenerates the paths with their jump counts and sizes.
 * model 0: Merton (GBM, sigma = 0.2): delta, gamma, vega, rho, theta, epsilon and the jump Greeks dlambda, dmu_j, dsigma_j;
 * model 1: Bates (Heston: v0 = theta = 0.04, kappa = 2, xi = 0.3, rho = -0.7; the reference's log-Euler scheme): delta
 * and gamma, the others are NaN.
 *
 *   gcc -O2 -I include examples/american_jump_greeks.c -o /tmp/american_jump_greeks \
 *       -L options_model_amd/lib -lomc -lm -Wl,-rpath,$PWD/options_model_amd/lib
 *   /tmp/american_jump_greeks [n_paths] [n_steps] [model: 0 GBM, 1 Heston] [lambda] [mu_j] [sigma_j] [yield] [bump] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "omc_jump_greeks.h"

int main(int argc, char** argv)
{
    const long long n_paths = argc > 1 ? atoll(argv[1]) : 1000000;
    const int n_steps = argc > 2 ? atoi(argv[2]) : 252;
    const int heston = argc > 3 ? atoi(argv[3]) : 0;
    omc_jump j;
    j.lambda = argc > 4 ? atof(argv[4]) : 1.0;
    j.mu_j = argc > 5 ? atof(argv[5]) : -0.1;
    j.sigma_j = argc > 6 ? atof(argv[6]) : 0.15;
    const double q = argc > 7 ? atof(argv[7]) : 0.0;
    const double bump = argc > 8 ? atof(argv[8]) : 0.01;
    omc_params p;
    memset(&p, 0, sizeof p);
    p.model = heston ? OMC_MODEL_HESTON : OMC_MODEL_GBM;
    p.heston_scheme = OMC_HESTON_REFERENCE_CLAMP;
    p.is_put = 1;
    p.semantics = OMC_SEM_TWO_PASS;
    p.antithetic = 1;
    p.n_paths = n_paths / 2 * 2;
    p.n_steps = n_steps;
    p.S0 = 100.0; p.K = 100.0; p.r = 0.05; p.sigma = 0.2; p.T = 1.0;
    p.v0 = 0.04; p.kappa = 2.0; p.theta = 0.04; p.xi = 0.3; p.rho = -0.7;
    p.seed = 42;
    omc_ctx* ctx = NULL;
    int rc = omc_ctx_create(0, NULL, &ctx);
    if (rc != 0) {
        fprintf(stderr, "omc_ctx_create: %d (%s)\n", rc, omc_last_error());
        return 1;
    }
    omc_jump_result quote;
    rc = omc_price_american_jump(ctx, &p, &j, q, &quote, NULL, 0);
    if (rc != 0) {
        fprintf(stderr, "omc_price_american_jump: %d (%s)\n", rc, omc_last_error());
        omc_ctx_destroy(ctx);
        return 1;
    }
    omc_jump_greeks out;
    rc = omc_price_american_jump_greeks(ctx, &p, &j, q, bump, NULL, NULL, &out);
    if (rc != 0) {
        fprintf(stderr, "omc_price_american_jump_greeks: %d (%s)\n", rc, omc_last_error());
        omc_ctx_destroy(ctx);
        return 1;
    }
    const omc_greeks* g = &out.g;
    printf("american %s put, %lld paths, %d steps, lambda %.3f, J ~ N(%.3f, %.3f^2), yield %.4f\n", heston ? "bates" : "merton",
           (long long)p.n_paths, n_steps, j.lambda, j.mu_j, j.sigma_j, q);
    printf("price %.6f (two-pass quote %.6f), %lld paths exercised early; %lld jumps drawn, kappa %.6f, drift rate %.6f\n",
           g->base.price, quote.base.price, (long long)g->base.n_exercised, (long long)out.n_jumps, out.kappa, out.drift_rate);
    printf("delta    %+.6f (se %.6f)\ngamma    %+.6f (se %.6f)   bump %.4f: price_up %.6f price_down %.6f\n", g->delta,
           g->se_delta, g->gamma, g->se_gamma, g->bump, g->price_up, g->price_down);
    printf("vega     %+.6f (se %.6f)\nrho      %+.6f (se %.6f)\ntheta    %+.6f (se %.6f), its score part %+.6f (se %.6f)\n", g->vega,
           g->se_vega, g->rho, g->se_rho, g->theta, g->se_theta, out.theta_score, out.se_theta_score);
    printf("epsilon  %+.6f (se %.6f)\ndlambda  %+.6f (se %.6f)\ndmu_j    %+.6f (se %.6f)\ndsigma_j %+.6f (se %.6f)\n", out.epsilon,
           out.se_epsilon, out.dlambda, out.se_dlambda, out.dmu_j, out.se_dmu_j, out.dsigma_j, out.se_dsigma_j);
    printf("kernels: paths %.3f ms, pass 1 %.3f ms, greeks sweep %.3f ms (the quote: paths %.3f ms, pass 2 %.3f ms)\n",
           g->base.ms_paths, g->base.ms_pass1, g->ms_greeks, quote.ms_jump_paths, quote.base.ms_pass2);
    omc_ctx_destroy(ctx);
    return 0;
}
