/* omc_dividend_bounds.h -- C ABI of libomc.so, the price bounds for a stock that pays discrete dividends: the dividend
 * generator as an entry point and Andersen-Broadie bounds under its law.  An extension header of
 * include/omc.h: it includes it, uses its structs (omc_params, omc_dividend, omc_bounds_config, omc_bounds) unchanged, and
 * adds two entry points; omc.h itself, OMC_ABI_VERSION (14) and every struct layout stay as they are. */
#ifndef OMC_DIVIDEND_BOUNDS_H
#define OMC_DIVIDEND_BOUNDS_H

#include "omc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Andersen-Broadie price bounds with discrete dividends: GBM and Heston ------------------ */
/* omc_dividend_paths_f32: the dividend generator of omc_price_american_div as an entry point, as omc_jump_paths_f32 is for
 * its law.  It writes the full-storage matrix S [n_steps+1][ld] (device, borrowed) of p->n_paths antithetic paths at
 * (p->seed, p->stream, p->pair_offset), started at (p->S0, p->v0), at the drift rate p->r - q, by exactly the step rule of
 * the section "dividends" of omc.h: the model's own step, then on a dividend step s = max(fma(s, mul, -cash), 0) for both
 * partners, so a row holds the EX-dividend spot.
 * step_offset in [0, n_steps]: row k takes the schedule's entry of step step_offset + k; steps beyond n_steps have none.
 *   It is the date the paths start at: row 0 is the start state as given and no entry is applied to it.  With
 *   step_offset = 0 and n_div > 0, S has the bits of omc_price_american_div's S_keep at the same arguments; with n_div = 0
 *   (or no entry behind step_offset) it writes the vanilla matrix (omc_gbm_paths_f32 / omc_heston_paths_f32) at rate
 *   p->r - q.
 * V: NULL, or (Heston only) device [n_steps+1][ld]: both partners' variance state after every step, row 0 = (float)v0,
 *   as omc_heston_paths_sv_f32 stores it (a dividend leaves the variance untouched).  S does not depend on whether V is
 *   given.
 * p->v0 is a start STATE for Heston schemes 0 .. 2 and is not validated: a stored full-truncation state may be negative,
 *   as in omc_heston_paths_from_normals_f32.  OMC_HESTON_QE keeps its v0 >= 0 check.  p->S0 is a start state as well and
 *   may be exactly 0, the spot a cash dividend larger than the spot leaves: such a path stays at 0.  p->semantics, K and
 *   is_put are not used beyond the omc_params checks.  The call returns when the matrices are written.
 * Errors (nothing is launched): the omc_params checks; -17 .. -24 as omc_price_american_div; -7 null ctx / S, or V given
 * with GBM; -6 ld < n_paths; -41 step_offset outside [0, n_steps].
 *
 * omc_price_american_bounds_div: omc_price_american_bounds with the dividend law.  p->model = OMC_MODEL_GBM, or
 * OMC_MODEL_HESTON with scheme OMC_HESTON_REFERENCE_CLAMP / OMC_HESTON_FULL_TRUNCATION (else -12); q, d and n_div as in
 * omc_price_american_div.  The game is Z_t = exp(-r t dt) max(phi(S_t), 0), t = 1..N, with S_t the EX-dividend spot of
 * row t: exercising at step k earns the ex-dividend payoff, the last cum-dividend exercise date is k - 1.  The policy table
 * betas [N+1][4], the stopping rule, the exercise tables, the outer walk, the sums, the standard errors, ci_*, the
 * outputs, the argument list from cfg on and ms_* are those of the section "price bounds for American options" of omc.h,
 * word for word; every discount factor is at p->r, the paths drift at p->r - q.  One GPU.  p->semantics is not used.
 * What the policy sees: the SPOT alone; cfg->regressors must be 0 (else -4).  The fitted policies are omc_lsm_poly's fits
 *   with semantics cfg->policy on omc_dividend_paths_f32's matrix of p->n_paths paths at (p->seed, p->stream,
 *   p->pair_offset); OMC_POLICY_GIVEN takes the caller's table.
 * What the bounds bound: the Bermudan game of the discretised law on the grid.  The schedule is deterministic, so the
 *   Markov state on a date is the spot (GBM) or (spot, variance) (Heston) together with the date; the inner paths start
 *   from that state AND from the date, and upper is an upper bound on the value of that game under any policy, biased
 *   upward only.  lower is what the spot-only policy earns in it.
 * Lower bound: the n_lower paths of omc_dividend_paths_f32 at stream cfg->stream_lower, pair offset 0.
 * Outer paths: omc_dividend_paths_f32(n_outer, ..) at cfg->stream_outer, pair offset 0, with the variance state kept under
 *   Heston: S_t[i], V_t[i].
 * Inner paths: inner pair j' of item (i, t) is generator pair g = (i (N+1) + t) (n_inner/2) + j' of cfg->stream_inner.  Its
 *   spots are bit for bit rows 0 .. N-t of omc_dividend_paths_f32(n_paths = n_inner, n_steps = N, T, S0 = S_t[i],
 *   v0 = V_t[i], step_offset = t, stream_inner, pair_offset = g).  The entry of step t itself is not applied again: row t
 *   of the outer matrix already holds the ex-dividend spot.  A spot of exactly 0 (a cash dividend larger than the spot)
 *   stays 0; items started there are legal.
 * Launches of at most 2^30 (GBM) / 2^29 (Heston) worst-case inner path steps.  Option "pass2_tables_irregular_every" acts
 *   as in omc_price_american_bounds.  float64 sums in a fixed order: identical calls return identical bits.
 * Options: "bounds_exercise_every" = k >= 2 (an exercise schedule) and "bounds_suboptimality" = 1 (the payoff check) are
 *   taken, each with exactly the semantics omc.h states; together they are refused with -40 as everywhere.
 *   "bounds_control_variate" = 1 is refused with -39 (the Black-Scholes control is not the European value after a cash
 *   dividend) and "bounds_suboptimality" = 2 with -40 (no European table), both after the call's own checks, with nothing
 *   launched and the outputs untouched.
 * Degenerate laws: with q = 0 and either n_div = 0 or every amount 0, every output but the timings carries the bits of
 *   omc_price_american_bounds (GBM) or of omc_price_american_bounds_heston with OMC_HESTON_REG_SPOT (Heston) at the same
 *   arguments: fmaxf(fmaf(s, 1, -0), 0) = s for s >= 0.
 * Errors (nothing is launched): -7 null ctx / cfg / out; the omc_params checks; -17 .. -24 as omc_price_american_div; -12
 * a Heston scheme other than 0 and 1; -4 cfg->regressors not 0; then -10, -4, -7, -3, -16 as omc_price_american_bounds;
 * then -39 / -40 as stated under Options. */
int omc_dividend_paths_f32(omc_ctx* ctx, const omc_params* p, double q, const omc_dividend* d, int n_div,
                           int step_offset, float* S, float* V /* NULL, or [n_steps+1][ld] for Heston */, int64_t ld);
int omc_price_american_bounds_div(omc_ctx* ctx, const omc_params* p, double q, const omc_dividend* d, int n_div,
                                  const omc_bounds_config* cfg, const double* betas, double* betas_out,
                                  double* q_out, double* samples_out, omc_bounds* out);

#ifdef __cplusplus
}
#endif

#endif /* OMC_DIVIDEND_BOUNDS_H */
