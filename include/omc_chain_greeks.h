/* omc_chain_greeks.h -- C ABI of libomc.so, the frozen-policy pathwise Greeks of a whole option chain, Bermudan entries
 * included, from one set of paths.  An extension header of include/omc.h: it includes it, uses its
 * structs (omc_params, omc_chain_entry, omc_greeks) unchanged, and adds one entry point and one info struct; omc.h itself,
 * OMC_ABI_VERSION (14) and every struct layout stay as they are. */
#ifndef OMC_CHAIN_GREEKS_H
#define OMC_CHAIN_GREEKS_H

#include "omc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* omc_price_american_chain_greeks: the Greeks of n quotes of ONE expiry -- strikes, sides and exercise schedules in e[],
 * everything else in p (p->K and p->is_put are ignored) -- from one generator launch and one path matrix, as
 * omc_price_american_chain prices them.  GBM and Heston at every scheme (0 .. 3), antithetic pairs, the two-pass flow, one
 * GPU; storage is chosen as by the single call (option "fold_antithetic").
 * betas: NULL (every entry's policy is the fit pass 1 makes on the shared paths), or host [n][n_steps+1][4]: one given policy
 *   per entry, as omc_price_american_greeks takes one; pass 1 is then skipped for all entries.  Of a Bermudan entry's given
 *   table the rows at its scheduled dates are read.  betas_out: NULL or host [n][n_steps+1][4], the policies used.
 * THE CONTRACT
 *   1. An American entry (exercise_every 0 or 1): out[i] equals omc_price_american_greeks(ctx, p with K = e[i].K and is_put
 *      = e[i].is_put, bump, slice i of betas, ..) BIT FOR BIT -- every field of `base` but ms_* and timed, every Greek and
 *      standard error, price_up / _down, n_exercised_up / _down -- and slice i of betas_out is that call's betas_out,
 *      whatever else the chain holds, in whatever order, at any "chain_greeks_k", on both storages.
 *   2. A Bermudan entry (exercise_every = k >= 2; the schedule of omc_price_american_chain, anchored at expiry): slice i of
 *      betas_out is what omc_price_american_chain returns for the entry -- the American fits' bits at the scheduled dates,
 *      zero elsewhere (given policies: the caller's rows at the scheduled dates, zero elsewhere) -- and out[i] equals, bit
 *      for bit, omc_price_american_greeks(ctx, p with e[i], bump, betas = that slice, ..): the single call with the masked
 *      policy GIVEN, which walks all rows and exercises at none off the schedule.  Two exceptions: base.sum_nitm (here the
 *      sum over the scheduled dates, there 0) and the time fields.  With k >= n_steps there is no early date: the Greeks
 *      are the European ones of the flow, those of a given table whose every n is 0.  The sweep reads the scheduled rows only.
 *   3. Identical calls return identical bits; a duplicated entry returns identical bits; a reversed chain returns the same
 *      bits per entry.
 *   4. Heston: vega, rho, theta and their standard errors are NaN, as in the single call.
 * Timings: out[i].base.ms_paths / ms_pass1 / ms_lsm / ms_total and out[i].ms_greeks repeat the chain's whole-call phases
 *   (info, below); base.timed is 1 for i = 0 only.
 * Errors (nothing is launched, the outputs are untouched), in this order: -7 null e; those of omc_price_american_chain for
 *   (p, e, n) in its order (p's own; -3 n < 1 or > OMC_CHAIN_MAX; -4 an entry's K or is_put, or p->semantics != 2; -15
 *   p->antithetic == 0; -37 a negative exercise_every; -10 a context with a communicator or an all-reduce hook); -4 bump
 *   outside (0, 0.5]; -7 null out.
 * Option "chain_greeks_k" (omc_set_option): entries of one side per Greeks sweep launch: -1 = default (16), 1 .. 16; 1 =
 *   one launch per entry.  The results do not depend on it.  ("chain_greeks_order", measurement only: 0 = default, the
 *   entries of 8 neighbouring column blocks dispatched together; 1 = entry slowest.  Nor do the results depend on it.) */
typedef struct {
    int32_t folded;             /* 1 = antithetic-folded storage                                                   */
    int32_t n_groups;           /* ceil(n / 16): groups whose reductions, solves and finalizes share one launch each */
    int32_t n_sweep_launches;   /* Greeks sweep launches of the call                                               */
    int32_t entries_per_launch; /* entries of one side a sweep launch takes at most                                */
    double ms_paths, ms_pass1, ms_greeks, ms_total; /* HIP-event times: the generator; pass-1 sweeps + reductions; solves +
                                                       Greeks sweeps + finalizes; first launch to last completion (with
                                                       the tables built in front of the generator)                  */
} omc_chain_greeks_info;
int omc_price_american_chain_greeks(omc_ctx* ctx, const omc_params* p, const omc_chain_entry* e, int n, double bump,
                                    const double* betas, double* betas_out, omc_greeks* out,
                                    omc_chain_greeks_info* info);

#ifdef __cplusplus
}
#endif

#endif /* OMC_CHAIN_GREEKS_H */
