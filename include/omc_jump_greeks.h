/* omc_jump_greeks.h -- C ABI of libomc.so, the frozen-policy Greeks of American options under jump-diffusion: Merton
 * (GBM) and Bates (Heston) with a continuous dividend yield.  An extension header of
 * include/omc.h: it includes it, uses its structs (omc_params, omc_jump, omc_greeks) unchanged, and adds one entry point;
 * omc.h itself, OMC_ABI_VERSION (14) and every struct layout stay as they are. */
#ifndef OMC_JUMP_GREEKS_H
#define OMC_JUMP_GREEKS_H

#include "omc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* omc_price_american_jump_greeks: the hedge ratios of the product omc_price_american_jump prices.  p, j and q are those of
 * omc_price_american_jump, with its checks and codes (omc_jump_table's); one GPU, p->semantics == OMC_SEM_TWO_PASS,
 * antithetic pairs.
 * Paths: the jump generator fills a FULL-storage matrix in the library's own buffer: g.base.folded is always 0.  At
 *   lambda = 0 no count word passes a threshold and the matrix is the vanilla generator's at rate p->r - q.
 * Policy: the fits pass 1 makes on that matrix, or `betas` (host [n_steps+1][4] = b0, b1, b2, n with the layout and
 *   meaning omc_price_american_greeks gives them: n <= 0 means no exercise at that step, so an all-n <= 0 table gives the
 *   Greeks of the European option; paths and pass 1 are then skipped and g.base.sum_nitm = 0).  betas_out (NULL or host
 *   [n_steps+1][4]) receives the policy used.
 * Sweep: ONE forward sweep on REGENERATED paths (it reads no matrix): the generator's own normals, count words, counts
 *   n = #{w >= thr[k]} and log2 jumps.  Per path three scenarios, started at (float)S0, (float)(S0 (1 + bump)) and
 *   (float)(S0 (1 - bump)), driven by the same growth factor of every step (GBM exp2(fma(+-b, z, a) + jl); Heston the
 *   scheme's factor, then exp2(jl)).  The base scenario's spots are bit for bit the generator's; the bumped ones are those
 *   of omc_price_american_jump at that S0.  Each scenario follows the frozen fits with pass 2's decision expression on its
 *   own spot; its exercise step k is the one pass 2 keeps -- the latest step in 1 .. N-1 at which the rule fires, N when
 *   it never does -- and s its spot there.
 *   It replaces pass 2: g.base.ms_pass2 = 0, g.ms_greeks is the sweep alone; g.base.n_exercised, n_zero and sum_nitm equal
 *   omc_price_american_jump's, and the price differs from it only in the order of its float64 sum.
 * Running sums of a pair (eps = +-1 the antithetic partner): W_k = sqrt(dt) sum_{j<=k} z_j (the partner's with the
 *   opposite sign), Nc_k = sum_{j<=k} n_j, ZJ_k = sum_{j<=k} sqrt(n_j) z_{J,j}, and the whole path's count N_tot = Nc_N.
 * Per path, with D_k = exp(-r (k-1) dt), cf = D_k max(phi(s), 0), phi' = -1{phi > 0} (put) / +1{phi > 0} (call),
 *   t_k = k dt, rj the drift rate, kappa' = kappa + 1 = exp(mu_j + sigma_j^2 / 2):
 *   delta    D_k phi' s / S0;  gamma (delta+ - delta-) / (2 bump S0) from the bumped scenarios' own stops, each delta
 *            D_k phi' Y with Y the float32 product of the partner's growth factors up to that stop: s / S0 of that
 *            scenario, formed once for both so that chains stopping together contribute exactly 0;
 *   vega     D_k phi' s (-sigma t_k + eps W_k);  rho -(k-1) dt cf + D_k phi' s t_k;  epsilon (dV/dq) -D_k phi' s t_k;
 *   dmu_j    D_k phi' s (Nc_k - lambda t_k kappa');  dsigma_j D_k phi' s (ZJ_k - lambda t_k sigma_j kappa');
 *   dlambda  D_k phi' s (-kappa t_k) + cf (N_tot / lambda - T);
 *   theta    -[-r (k-1)/N cf + D_k phi' s ((rj - sigma^2/2) k/N + eps sigma W_k / (2T)) + cf (N_tot / T - lambda)]:
 *            -dV/dT at fixed n_steps;  theta_score = -cf (N_tot / T - lambda), the part of theta that is no pathwise term.
 *   A step's jump count is an integer, so dlambda and theta need a score-function (likelihood-ratio) term next to their
 *   pathwise part.  The score uses the WHOLE path's count and not the count up to k: k is the latest fire and therefore
 *   no stopping time, so only the full path's likelihood ratio is valid.  The terms are the derivatives of
 *   prod_j Poisson(n_j; x), x = lambda T / N, in lambda and in T.  The sampled law is the 24-bit quantised one, truncated
 *   at 16 jumps; its score differs from this one by O(2^-24) per step, far below any standard error.
 * Heston (Bates; every scheme, OMC_HESTON_QE included): delta and gamma; every other Greek and its standard error are
 *   NaN.  lambda = 0: dmu_j, dsigma_j and theta_score are exactly 0; dlambda and its standard error are NaN (the score is
 *   undefined at 0).  Standard errors as omc_price_american_greeks.  float64 sums in a fixed order: identical calls return
 *   identical bits.
 * Errors (nothing is launched, *out untouched): -7 null ctx / out; those of omc_price_american_jump (the omc_params
 * checks, -25, -17, -26, -27, -28, -24, -11); -4 bump outside (0, 0.5] (NaN included); -10 a distributed context. */
typedef struct {
    omc_greeks g;                       /* base, delta .. theta, se_*, bump, price_up/down, n_exercised_up/down, ms_greeks */
    double epsilon, se_epsilon;         /* dV/dq                                                                           */
    double dlambda, se_dlambda;         /* dV/dlambda: pathwise drift part + score part                                    */
    double dmu_j, se_dmu_j;             /* dV/dmu_j, pathwise                                                              */
    double dsigma_j, se_dsigma_j;       /* dV/dsigma_j, pathwise                                                           */
    double theta_score, se_theta_score; /* the score part of theta alone (already inside g.theta)                          */
    double kappa, drift_rate;           /* as omc_jump_result                                                              */
    int64_t n_jumps;                    /* jumps drawn over all pairs and steps                                            */
} omc_jump_greeks;
int omc_price_american_jump_greeks(omc_ctx* ctx, const omc_params* p, const omc_jump* j, double q, double bump,
                                   const double* betas, double* betas_out, omc_jump_greeks* out);

#ifdef __cplusplus
}
#endif

#endif /* OMC_JUMP_GREEKS_H */
