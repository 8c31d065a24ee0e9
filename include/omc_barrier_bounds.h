/* omc_barrier_bounds.h -- C ABI of libomc.so, the price bounds for barrier options: the barrier generator that keeps the
 * paths' state as an entry point and Andersen-Broadie bounds under the barrier law.  An extension
 * header of include/omc.h: it includes it, uses its structs (omc_params, omc_barrier, omc_bounds_config, omc_bounds)
 * unchanged, and adds two entry points; omc.h itself, OMC_ABI_VERSION (14) and every struct layout stay as they are. */
#ifndef OMC_BARRIER_BOUNDS_H
#define OMC_BARRIER_BOUNDS_H

#include "omc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Andersen-Broadie price bounds for knock-in / knock-out options: GBM and Heston ---------- */
/* The contract is that of the section "barrier options" of omc.h with OMC_MONITOR_DISCRETE: the four OMC_BARRIER_* kinds;
 * a partner is hit at step t = 1..N when its float32 spot passes the exact float32 threshold of H; a knock-out is dead AT
 * its hit step and after it, a knock-in is live FROM its hit step on and its row 0 is dead; where the option is not live
 * the ENCODED index holds the dead spot, the float32 nearest K on its out-of-the-money side; no rebate.  b->american is
 * not read.
 *
 * omc_barrier_paths_state_f32: the barrier generator with the state of every path kept.  p->n_paths antithetic paths at
 * (p->seed, p->stream, p->pair_offset), started at (p->S0, p->v0); p->model = OMC_MODEL_GBM, or OMC_MODEL_HESTON with scheme
 * OMC_HESTON_REFERENCE_CLAMP / OMC_HESTON_FULL_TRUNCATION.  All matrices are device memory, borrowed, [n_steps+1][ld]:
 *   E    the encoded index.  With start_hit = 0 it has the bits of omc_price_barrier's S_keep at the same arguments.
 *   S    the real spots: the bits of omc_gbm_paths_f32 / omc_heston_paths_f32.
 *   V    Heston: both partners' variance state after every step as omc_heston_paths_sv_f32 stores it; GBM: must be NULL.
 *   hit  device int32 [n_paths]: the first step at which the path is hit, 0 = never.  The flag is monotone: path i is hit
 *        at date t iff hit[i] != 0 && hit[i] <= t.
 * start_hit: 0, the paths start not hit and S0 on or beyond the barrier is refused (-14); 1, a restart from a state that
 *   has been hit before: row 0 is encoded as hit, every entry of hit is -1 (the rule above still holds), and S0 may lie
 *   anywhere.  p->v0 of a Heston call is a start STATE and is not validated (a stored full-truncation state may be negative).
 * The call returns when the matrices are written.
 * Errors (nothing is launched): the omc_params checks; -7 null ctx / b / E / S / hit, V missing under Heston or given under
 * GBM; -15 unknown kind or monitoring, start_hit not 0 / 1, antithetic = 0; -12 continuous monitoring, a Heston scheme other
 * than 0 and 1; -13 H not finite and positive; -14 (start_hit = 0) S0 on or beyond the barrier; -10 a distributed context;
 * -6 ld < n_paths.
 *
 * omc_price_american_bounds_barrier: omc_price_american_bounds for the American barrier option omc_price_barrier quotes.
 * The game is Z_t = exp(-r t dt) max(phi(X_t), 0), t = 1..N, X_t the encoded index of row t: a live option pays the vanilla
 * payoff, a dead one nothing.  The policy table betas [N+1][4], the exercise tables, the outer walk, the sums, the standard
 * errors, ci_*, the outputs, the argument list from cfg on and ms_* are those of the section "price bounds for American
 * options" of omc.h, word for word, ON THE ENCODED INDEX: a dead index never exercises.  One GPU.  p->semantics is not
 * used; cfg->regressors must be 0 (else -4).
 * The state of a path on a date is (spot, hit yes / no[, variance]): paths step on the REAL spot, the policy sees the index.
 * Policy: omc_lsm_poly's fits with semantics cfg->policy on omc_price_barrier's encoded matrix of p->n_paths paths at
 *   (p->seed, p->stream, p->pair_offset); OMC_POLICY_GIVEN takes the caller's table.
 * Lower bound: the n_lower paths of omc_barrier_paths_state_f32 at stream cfg->stream_lower, pair offset 0.  Each partner
 *   stops at the first date the policy exercises its index.  A knocked-out partner stops, with value 0, at the first
 *   exercise date at or after its hit step -- without a schedule the hit step itself; its stop date enters
 *   n_exercised_lower (and, for inner paths, inner_path_steps) exactly as an exercise at that date would.
 * Outer paths: omc_barrier_paths_state_f32(n_outer, ..) at cfg->stream_outer, pair offset 0: E_t[i], S_t[i], V_t[i], hit[i].
 * Inner paths: inner pair j' of item (i, t) is generator pair g = (i (N+1) + t) (n_inner/2) + j' of cfg->stream_inner.  Its
 *   index is bit for bit rows 0 .. N-t of omc_barrier_paths_state_f32(n_paths = n_inner, n_steps = N, T, S0 = S_t[i],
 *   v0 = V_t[i], start_hit = hit(t, i), stream_inner, pair_offset = g), its stopping rule the lower bound's.  A knock-in
 *   that has not hit keeps monitoring behind the dead spot.  An item of a knock-out that is dead at t is not simulated:
 *   Q^[i][t] = 0.0 exactly and it adds no steps.
 * Options: "bounds_exercise_every" = k >= 2 is taken: monitoring stays on every step of the grid, exercise is on the
 *   scheduled dates.  "bounds_suboptimality" = 1 (the payoff check) is taken; it drops every dead item by construction.
 *   Refused with -12, after the call's own checks, nothing launched and the outputs untouched: "bounds_suboptimality" = 2
 *   (a vanilla European value is no bound on a barrier continuation value) and "bounds_control_variate" = 1.  Schedule and
 *   payoff check together are refused with -40 as everywhere.
 * Degenerate contracts: a knock-out whose barrier no path reaches returns, in every output but the timings, the bits of
 *   omc_price_american_bounds (GBM) / omc_price_american_bounds_heston with OMC_HESTON_REG_SPOT (Heston) at the same
 *   arguments; a knock-in whose barrier no path reaches returns lower = upper = 0 with both standard errors 0.
 * Errors (nothing is launched): -7 null ctx / cfg / out / b; the omc_params checks; -15 unknown kind or monitoring,
 * antithetic = 0; -12 continuous monitoring, a Heston scheme other than 0 and 1; -13; -14; -4 cfg->regressors not 0; -12 the
 * two options above; then -10, -4, -7, -3, -16, -40 as omc_price_american_bounds. */
int omc_barrier_paths_state_f32(omc_ctx* ctx, const omc_params* p, const omc_barrier* b, int start_hit, float* E, float* S,
                                float* V /* NULL for GBM, [n_steps+1][ld] for Heston */, int32_t* hit, int64_t ld);
int omc_price_american_bounds_barrier(omc_ctx* ctx, const omc_params* p, const omc_barrier* b,
                                      const omc_bounds_config* cfg, const double* betas, double* betas_out, double* q_out,
                                      double* samples_out, omc_bounds* out);

#ifdef __cplusplus
}
#endif

#endif /* OMC_BARRIER_BOUNDS_H */
