/* omc_dividend_greeks.h -- C ABI of libomc.so, the frozen-policy pathwise Greeks of American options on a stock that pays
 * a dividend yield and discrete dividends.  An extension header of include/omc.h: it includes it,
 * uses its structs (omc_params, omc_dividend, omc_greeks) unchanged, and adds one entry point; omc.h itself,
 * OMC_ABI_VERSION (14) and every struct layout stay as they are. */
#ifndef OMC_DIVIDEND_GREEKS_H
#define OMC_DIVIDEND_GREEKS_H

#include "omc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* omc_price_american_div_greeks: the hedge ratios of the product omc_price_american_div prices.  p, q, d and n_div are
 * those of omc_price_american_div, with its checks, codes and per-step table (omc_dividend_schedule); one GPU,
 * p->semantics == OMC_SEM_TWO_PASS, antithetic pairs.
 * Paths: the dividend generator (omc_dividend_paths_f32 at step_offset 0) fills a FULL-storage matrix in the library's own
 *   buffer: g.base.folded is always 0, and with n_div = 0 the matrix is the vanilla generator's at rate p->r - q.
 * Policy: the fits pass 1 makes on that matrix, or `betas` (host [n_steps+1][4] = b0, b1, b2, n with the layout and
 *   meaning omc_price_american_greeks gives them: n <= 0 means no exercise at that step, so an all-n <= 0 table gives the
 *   Greeks of the European option; paths and pass 1 are then skipped and g.base.sum_nitm = 0).  betas_out (NULL or host
 *   [n_steps+1][4]) receives the policy used.
 * Sweep: ONE forward sweep on REGENERATED paths (it reads no matrix): per path three scenarios, started at (float)S0,
 *   (float)(S0 (1 + bump)) and (float)(S0 (1 - bump)), driven by the same normals and the same growth factor of every step,
 *   each through s = fmaxf(fmaf(s, mul, -cash), 0) on the dividend steps.  The base scenario's spots are bit for bit the
 *   generator's; the bumped ones are those of omc_price_american_div at that S0.  Each scenario follows the frozen fits with
 *   pass 2's decision expression on its own spot; its exercise step k is the one pass 2 keeps -- the latest step in
 *   1 .. N-1 at which the rule fires, N when it never does -- and s its ex-dividend spot there.
 *   It replaces pass 2: g.base.ms_pass2 = 0, g.ms_greeks is the sweep alone; g.base.n_exercised, n_zero and sum_nitm equal
 *   omc_price_american_div's, and the price differs from it only in the order of its float64 sum.
 * Tangents (eps = +-1 the antithetic partner, G the step's growth factor, Sm = S G the cum-dividend spot, float32):
 *   Y  <- Y G, Y_0 = 1 (every scenario; dS/dS0);  GBM, base scenario:  Ys <- Ys G + Sm (-sigma dt + eps sqrt(dt) z),
 *   Yr <- Yr G + Sm dt,  YT <- YT G + Sm ((r - q - sigma^2/2)/N + eps sigma z / (2 sqrt(T N)));  dS/dq = -Yr.
 *   On a dividend step every tangent becomes mul Y where the ex-dividend spot is positive and 0 where the floor took it.
 * Per path, with D_k = exp(-r (k-1) dt), cf = D_k max(phi(s), 0), phi' = -1{phi > 0} (put) / +1{phi > 0} (call):
 *   delta D_k phi' Y;  vega D_k phi' Ys;  rho -(k-1) dt cf + D_k phi' Yr;  epsilon (dV/dq) -D_k phi' Yr;
 *   theta -[-r (k-1)/N cf + D_k phi' YT]: -dV/dT at fixed n_steps with the dividends fixed on their STEPS and at their
 *   amounts;  gamma (delta+ - delta-) / (2 bump S0) from the bumped scenarios' own stops and own Y.
 *   price_up / price_down / n_exercised_up / _down as omc_price_american_greeks.  No sensitivity to a dividend amount.
 * Heston (every scheme, OMC_HESTON_QE included): delta and gamma; vega, rho, theta, epsilon and their standard errors are
 *   NaN.  Standard errors as omc_price_american_greeks.  float64 sums in a fixed order: identical calls return identical
 *   bits.  Without discrete dividends and with q = 0 the terms are omc_price_american_greeks' closed forms.
 * Errors (nothing is launched): -7 null ctx / out; those of omc_price_american_div (the omc_params checks, -17 .. -24,
 * -11); -4 bump outside (0, 0.5] (NaN included); -10 a distributed context. */
typedef struct {
    omc_greeks g;                 /* base, delta .. theta, se_*, bump, price_up/down, n_exercised_up/down, ms_greeks */
    double epsilon, se_epsilon;   /* dV/dq                                                                           */
    int32_t n_div_steps;          /* time steps on which at least one dividend goes ex (0: yield only)               */
    int32_t first_div_step;       /* the first of them (0: none)                                                     */
} omc_div_greeks;
int omc_price_american_div_greeks(omc_ctx* ctx, const omc_params* p, double q, const omc_dividend* d, int n_div,
                                  double bump, const double* betas, double* betas_out, omc_div_greeks* out);

#ifdef __cplusplus
}
#endif

#endif /* OMC_DIVIDEND_GREEKS_H */
