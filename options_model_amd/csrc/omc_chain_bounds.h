// omc_chain_bounds.h -- host interface of the chain bound kernels (omc_chain_bounds.hip): the lower
// sweep and the inner simulations of omc_bounds.hip with up to kChainBoundsMax frozen policies riding on ONE simulation of
// every fresh path.
#pragma once
#include "omc_bounds.h"

namespace omc {

// Entries per launch at most.  8, not 4: the inner kernel already runs 3 waves per SIMD at 4 entries (131 vector registers,
// GBM) and still does at 8 (162), with no scratch at either, so the longer group costs no occupancy and halves the inner
// simulations of a long chain; its tables take 8 x 16 (N+1) bytes of LDS (profiles/chain_bounds_resource_usage.txt).
constexpr int kChainBoundsMax = 8;
// LDS a workgroup takes for the entries' exercise tables at most (what a launch may ask for without an attribute)
constexpr size_t kChainBoundsLds = 65536;

// what differs between the entries of a group; everything else is the call's BoundsArgs
struct ChainBoundsEntry {
    double K, invK;
    const double* betas;        // [N+1][4] the entry's policy (float64 rule on irregular dates)
    const uint32_t* tab;        // [N+1][8] its exercise tables (lsm_crit_build)
    double* q;                  // [n_outer][N] its Q^_t
    double* samples;            // [n_outer]
    double* part;               // [8][kPStride] its per-workgroup partials
    unsigned long long* steps;  // its inner path steps: the single call's count
    int is_put, pad_;
};
struct ChainBoundsGroup {
    int E, pad_;
    unsigned long long* steps_sim;  // steps simulated: per partner the LARGEST stop date of the group's entries
    ChainBoundsEntry e[kChainBoundsMax];
};

// entries per group for N dates: the tables uint4 [E][N+1] within kChainBoundsLds, at least 1, at most kChainBoundsMax
inline int chain_bounds_group_max(int N)
{
    const size_t fit = kChainBoundsLds / bounds_table_lds(N);
    return fit < 1 ? 1 : (fit > (size_t)kChainBoundsMax ? kChainBoundsMax : (int)fit);
}
// entry e of the group as the single kernels' argument block: what the walk and the table builder take
BoundsArgs chain_bounds_entry_args(const BoundsArgs& a, const ChainBoundsEntry& e);

// The lower sweep of every entry on one set of lower pairs: result[e] (8 doubles each, device) <- the sums of
// bounds_lower for that entry, bit for bit.  l: model 0 (GBM) or Heston scheme 0 / 1; else hipErrorInvalidValue, as is a
// group that is empty, too long for kChainBoundsMax or too long for its tables' LDS.
hipError_t chain_bounds_lower(hipStream_t st, const BoundsArgs& a, const DiffusionLaw& l, const ChainBoundsGroup& g,
                              double* const* result);
// Q^_t[i] of every entry for outer paths [i0, i0 + ni) and t = 0..N-1 from one simulation of each inner pair
hipError_t chain_bounds_inner(hipStream_t st, const BoundsArgs& a, const DiffusionLaw& l, const ChainBoundsGroup& g, int64_t i0,
                              int64_t ni);

}  // namespace omc
