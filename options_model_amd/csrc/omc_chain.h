// omc_chain.h -- host-callable launchers of the option-chain kernels (omc_chain.hip; internal to libomc.so): many strikes and
// sides of one expiry priced from ONE path matrix (omc_price_american_chain).
#pragma once
#include "omc_kernels.h"

namespace omc {

constexpr int kChainGroupMax = 16;  // entries per group: their pass-1 reductions, table builds and finalizes share one
                                    // launch each (lsm_group_*, omc_kernels.h)
constexpr int kChainWidthMax = 4;   // entries of one side per fused sweep launch

// cK_j[t] = c0[j] g^t, t = 0 .. N, for j < n: table j at cK + j * stride, each filled as lsm_fold_table fills its one
// (fold_table_fill; c0: device, n doubles)
hipError_t chain_fold_tables(hipStream_t st, double* cK, size_t stride, const double* c0, int n, int N, double g);

// One fused launch: KE entries of ONE side on the folded matrix S ([N+1][ld], P stored columns).  Entry e reads its strike,
// its fold table and -- pass 2 -- its exercise tables and fits, and leaves its partial sums in its own slabs, in the
// geometry of the single kernels: part1[e] as lsm_pass1_sweep leaves w.part1, part[e] as lsm_pass2_sweep leaves w.part.
struct ChainSweepArgs {
    const float* S;
    int64_t ld, P;
    int N, KE, is_put, pad_;
    const double* D;
    double K[kChainWidthMax], invK[kChainWidthMax];
    const double* cK[kChainWidthMax];
    double* part1[kChainWidthMax];
    const uint32_t* crit[kChainWidthMax];
    const double* betas[kChainWidthMax];
    double* part[kChainWidthMax];
};
// Whether the fused sweeps cover the folded problem p (the geometry knobs of the single sweeps at their defaults) and how
// many entries one launch may take at most: 4, 2 or 1, bounded by the registers the per-entry state of pass 2 takes (entries
// x columns per thread <= 8) and by the LDS its tables need (32 bytes per step and entry); 0 = not covered.
int chain_fused_width(const LsmProblem& p);
// *ntiles / *nblk: what lsm_pass1_sweep / lsm_pass2_sweep report for the same problem
hipError_t chain_pass1_sweep(hipStream_t st, const ChainSweepArgs& a, const LsmProblem& p, int64_t* ntiles);
hipError_t chain_pass2_sweep(hipStream_t st, const ChainSweepArgs& a, const LsmProblem& p, int* nblk);

}  // namespace omc
