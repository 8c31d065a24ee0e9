/* omc_jump_bounds.h -- C ABI of libomc.so, the jump-diffusion price bounds: the jump generator as an entry point and
 * Andersen-Broadie bounds under Merton's and Bates's models.  An extension header of include/omc.h:
 * it includes it, uses its structs (omc_params, omc_jump, omc_bounds_config, omc_bounds) unchanged, and adds two entry
 * points; omc.h itself, OMC_ABI_VERSION (14) and every struct layout stay as they are. */
#ifndef OMC_JUMP_BOUNDS_H
#define OMC_JUMP_BOUNDS_H

#include "omc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Andersen-Broadie price bounds under jump-diffusion: Merton and Bates ------------------ */
/* omc_jump_paths_f32: the jump generator of omc_price_american_jump as an entry point, as omc_gbm_paths_f32 and
 * omc_heston_paths_sv_f32 are for their laws.  It writes the full-storage matrix S [n_steps+1][ld] (device, borrowed) of
 * p->n_paths antithetic paths at (p->seed, p->stream, p->pair_offset), started at (p->S0, p->v0), at the drift rate
 * (p->r - q) - lambda kappa, by exactly the step rule of the section "jump-diffusion" of omc.h.  For lambda > 0 S has the
 * bits of omc_price_american_jump's S_keep at the same arguments; lambda = 0 is allowed and writes the vanilla matrix
 * (omc_gbm_paths_f32 / omc_heston_paths_f32) at rate p->r - q.
 * V: NULL, or (Heston only) device [n_steps+1][ld]: both partners' variance state after every step, row 0 = (float)v0,
 *   as omc_heston_paths_sv_f32 stores it (a jump leaves the variance untouched).  S does not depend on whether V is given.
 * p->v0 is a start STATE for Heston schemes 0 .. 2 and is not validated: a stored full-truncation state may be negative,
 *   as in omc_heston_paths_from_normals_f32.  OMC_HESTON_QE keeps its v0 >= 0 check.  p->semantics, K and is_put are not
 *   used beyond the omc_params checks.  The call returns when the matrices are written.
 * Errors (nothing is launched): the omc_params checks; -25, -17, -26, -27, -28, -24 as omc_price_american_jump; -7 null
 * ctx / S, or V given with GBM; -6 ld < n_paths.
 *
 * omc_price_american_bounds_jump: omc_price_american_bounds with the jump law.  p->model = OMC_MODEL_GBM (Merton) or
 * OMC_MODEL_HESTON with scheme OMC_HESTON_REFERENCE_CLAMP / OMC_HESTON_FULL_TRUNCATION (Bates); j and q as in
 * omc_price_american_jump.  The game Z_t = exp(-r t dt) max(phi(S_t), 0), t = 1..N, the policy table betas [N+1][4], the
 * stopping rule, the exercise tables, the outer walk, the sums, the standard errors, ci_*, the outputs, the argument
 * list from cfg on and ms_* are those of the section "price bounds for American
 * options" of omc.h, word for word; every
 * discount factor is at p->r, the paths drift at rj = (p->r - q) - lambda kappa.  One GPU.  p->semantics is not used.
 * What the policy sees: the SPOT alone; cfg->regressors must be 0.  The fitted policies are omc_lsm_poly's fits with
 *   semantics cfg->policy on omc_jump_paths_f32's matrix of p->n_paths paths at (p->seed, p->stream, p->pair_offset);
 *   OMC_POLICY_GIVEN takes the caller's table.
 * What the bounds bound: the Bermudan game of the discretised law on the grid.  The jumps of a step are independent of
 *   the past, so the Markov state is the spot (Merton) or (spot, variance) (Bates); the inner paths start from it, and
 *   upper is an upper bound on the value of that game under any policy, biased upward only.  lower is what the spot-only
 *   policy earns in it.
 * Lower bound: the n_lower paths of omc_jump_paths_f32 at stream cfg->stream_lower, pair offset 0.
 * Outer paths: omc_jump_paths_f32(n_outer, ..) at cfg->stream_outer, pair offset 0, with the variance state kept under
 *   Heston: S_t[i], V_t[i].
 * Inner paths: inner pair j' of item (i, t) is generator pair g = (i (N+1) + t) (n_inner/2) + j' of cfg->stream_inner, and
 *   its inner step k = 1..N-t is step k of that generator pair: the pair's normal blocks, count block (k-1) >> 2 with tag
 *   0x40000000, size block with tag 0xC0000000 | k.  The inner spots are bit for bit rows 0 .. N-t of
 *   omc_jump_paths_f32(n_paths = n_inner, n_steps = N, T, S0 = S_t[i], v0 = V_t[i], stream_inner, pair_offset = g).  Both
 *   partners share count and jump size; only the diffusion is antithetic.
 * Launches of at most 2^30 (GBM) / 2^29 (Heston) worst-case inner path steps.  Option "pass2_tables_irregular_every" acts
 *   as in omc_price_american_bounds.  float64 sums in a fixed order: identical calls return identical bits.
 * Options: "bounds_exercise_every" = k >= 2 (an exercise schedule) and "bounds_suboptimality" = 1 (the payoff check) are
 *   taken, each with exactly the semantics omc.h states, the inner pairs started at the outer state and the fit on the
 *   gathered jump paths; together they are refused with -40 as everywhere.  "bounds_control_variate" = 1 is refused with -39
 *   (it would need Merton's series per item) and "bounds_suboptimality" = 2 with -40 (no European table), both after the
 *   call's own checks, with nothing launched and the outputs untouched.
 * Degenerate laws: with q = 0 and either lambda = 0, or mu_j = sigma_j = 0 at any admissible lambda > 0, every output but
 *   the timings carries the bits of omc_price_american_bounds (GBM) or of omc_price_american_bounds_heston with
 *   OMC_HESTON_REG_SPOT (Heston) at the same arguments: a zero-size jump adds exactly 0 to the exponent or multiplies by
 *   exp2(0) = 1.
 * Errors (nothing is launched): -7 null ctx / cfg / out; the omc_params checks; -25, -17, -26, -27, -28, -24 as
 * omc_price_american_jump; -12 a Heston scheme other than 0 and 1; -4 cfg->regressors not 0; then -10, -4, -7, -3, -16 as
 * omc_price_american_bounds; then -39 / -40 as stated under Options. */
int omc_jump_paths_f32(omc_ctx* ctx, const omc_params* p, const omc_jump* j, double q, float* S,
                       float* V /* NULL, or [n_steps+1][ld] for Heston */, int64_t ld);
int omc_price_american_bounds_jump(omc_ctx* ctx, const omc_params* p, const omc_jump* j, double q,
                                   const omc_bounds_config* cfg, const double* betas, double* betas_out, double* q_out,
                                   double* samples_out, omc_bounds* out);

#ifdef __cplusplus
}
#endif

#endif /* OMC_JUMP_BOUNDS_H */
