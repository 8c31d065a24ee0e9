/* omc_chain_bounds.h -- C ABI of libomc.so, the Andersen-Broadie price bounds of a whole option chain from one set of
 * fresh paths.  An extension header of include/omc.h: it includes it, uses its structs (omc_params,
 * omc_chain_entry, omc_bounds_config, omc_bounds) unchanged, and adds one entry point and one info struct; omc.h itself,
 * OMC_ABI_VERSION (14) and every struct layout stay as they are. */
#ifndef OMC_CHAIN_BOUNDS_H
#define OMC_CHAIN_BOUNDS_H

#include "omc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* omc_price_american_chain_bounds: out[i] = the bounds omc_price_american_bounds (p->model == OMC_MODEL_GBM) or
 * omc_price_american_bounds_heston with regressors spot (OMC_MODEL_HESTON, scheme reference or full truncation) returns for
 * p with K = entries[i].K and is_put = entries[i].is_put and the same cfg -- n_entries quotes of ONE expiry; p->K and
 * p->is_put are ignored, as in omc_price_american_chain.
 * Shared by all entries (they depend on neither the strike nor the side): the p->n_paths fitting paths, the lower-bound
 *   pairs, the outer paths and EVERY inner pair -- inner pair j of item (i, t) is generator pair (i (N+1) + t) (n_inner/2)
 *   + j of cfg->stream_inner, as in the single call.  Per entry: the policy (the fit of cfg->policy on the shared fitting
 *   paths, or slice i of `betas`), its exercise tables, its stops, its sums, its walk.
 * Groups: the entries run in groups of at most OMC_CHAIN_BOUNDS_MAX, fewer while the group's exercise tables
 *   (16 (N+1) bytes per entry) would not fit 65536 bytes of LDS (info->entries_per_group).  Within a group each lower pair and
 *   each inner pair is simulated ONCE, until its last entry has stopped; every group simulates the inner pairs again.
 * THE CONTRACT, entry by entry against its single call with the same sizes, seed and streams:
 *   betas_out, lower, se_lower, n_exercised_lower, inner_path_steps: equal bit for bit, at any sizes.
 *   q_out, samples_out, upper, se_upper: equal bit for bit while n_inner <= 128 (no lane of the inner sweep is refilled);
 *     beyond, they differ by the order of float64 sums of non-negative terms alone (measured: DESIGN.md 33.5).
 *   Option "pass2_tables_irregular_every" acts as in the single call.  Identical calls return identical bits.
 * betas: NULL, or with cfg->policy == OMC_POLICY_GIVEN host [n_entries][N+1][4].  betas_out: NULL or host
 *   [n_entries][N+1][4]; q_out: NULL or host [n_entries][n_outer][N]; samples_out: NULL or host [n_entries][n_outer].
 * out[i].ms_*: the chain's whole-call phase times, repeated in every entry.  info (may be NULL): see below.
 * Errors (nothing is launched, the outputs are untouched), in this order: -7 null ctx / p / entries / cfg / out; -42
 *   n_entries < 1 or > OMC_CHAIN_MAX; -4 an entry whose K is not finite and positive or whose is_put is not 0 / 1; the
 *   omc_params checks of omc_price_american for p; -46 a Heston scheme other than reference and full truncation; -4
 *   cfg->regressors != 0 (the policy sees the spot); -44 an entry with exercise_every != 0 (Bermudan entries have no chain
 *   bounds yet); -43 a context with a communicator or an all-reduce hook; -45 while one of the options
 *   "bounds_exercise_every" (>= 2), "bounds_control_variate", "bounds_suboptimality" is set; then -4 (policy), -7 (betas
 *   NULL with OMC_POLICY_GIVEN), -3 and -16 as omc_price_american_bounds. */
#define OMC_CHAIN_BOUNDS_MAX 8
typedef struct {
    int64_t inner_path_steps_simulated; /* per inner partner the LARGEST stop date over the entries of its group, minus the
                                           item's date, summed over all partners and groups: at least the largest and at
                                           most the sum of the entries' inner_path_steps                              */
    int32_t n_groups;                   /* ceil(n_entries / entries_per_group)                                         */
    int32_t entries_per_group;          /* min(OMC_CHAIN_BOUNDS_MAX, 65536 / (16 (N+1))), at least 1                   */
    double ms_fit, ms_lower, ms_upper, ms_total; /* HIP-event times: all fits; all lower sweeps; outer paths, tables, inner
                                                    sweeps, walks; the whole call                                    */
} omc_chain_bounds_info;
int omc_price_american_chain_bounds(omc_ctx* ctx, const omc_params* p, const omc_chain_entry* entries, int n_entries,
                                    const omc_bounds_config* cfg, const double* betas, double* betas_out, double* q_out,
                                    double* samples_out, omc_bounds* out, omc_chain_bounds_info* info);

#ifdef __cplusplus
}
#endif

#endif /* OMC_CHAIN_BOUNDS_H */
