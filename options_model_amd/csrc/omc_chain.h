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

// ---- Bermudan entries (omc_chain_entry::exercise_every = k >= 2)
// The scheduled dates of an N-step grid are t = N - k m >= 1, m = 1, 2, ...: n_e = (N - 1) / k of them.  Together with
// the expiry they are the rows 1 .. Nv = n_e + 1 of a VIEW of the path matrix with leading dimension k ld whose row j
// is the matrix's row N - k (Nv - j) (row 0 of the view lies above the matrix when k does not divide N: no sweep reads a
// row 0).  The two-pass flow with every unscheduled date skipped in both passes is the two-pass flow of that view -- the
// single pricing's own sweeps, which then touch the scheduled rows and no others -- once the three tables the sweeps
// index by row are restated on the view's rows:
//     pass 1 discounts a row's targets from expiry by D[N - t]              ->  d1[Nv - j] = D[k (Nv - j)]
//     pass 2 values an exercise at row t by D[t - 1]                        ->  d2[j - 1]  = D[N - k (Nv - j) - 1]
//     the fold table of the entry                                           ->  cv[j]      = cK[N - k (Nv - j)]
// gathered (copied, so they carry the bits of the tables every other entry reads) by one launch for the whole chain.
constexpr int kChainMax = 256;  // OMC_CHAIN_MAX
struct ChainSchedules {
    int every[kChainMax];  // per entry: k, already cut to 2 .. N; below 2 = every date (no tables)
};
__host__ __device__ inline int chain_view_steps(int N, int k) { return (N - 1) / k + 1; }  // Nv
// tables of entry i at out + 3 stride i: d1, d2, cv, each of `stride` >= N + 1 doubles (cv only when cK is given: the
// entries' fold tables, table i at cK + cstride i)
hipError_t chain_schedule_tables(hipStream_t st, double* out, size_t stride, const double* D, const double* cK,
                                 size_t cstride, const ChainSchedules& s, int n, int N);

// The one sweep that cannot take the view: pass 1 on FULL storage with 16-byte loads (lsm_pass1_kernel<4, ..>).  Its three
// unrolled row slots do not round alike -- the first forms the u^2 sum of its first two columns as fma(u0, u0, rnd(u1^2)),
// the other two as fma(u1, u1, rnd(u0^2)) -- so a date's moments depend on its position in its chunk, which the view
// changes: the fits would leave the American entry's in the last bits (seen at 1 date in ~20).  Such an entry's pass 1 is
// the American entry's own, over all rows, and this launch then moves the scheduled rows of its reduced moments to the
// view's rows: gmom[j] = gmom[N - k (Nv - j)], j = 1 .. Nv - 1, in place (ascending j: a source row is never below j).
struct ChainGatherArgs {
    double* gmom[kChainGroupMax];  // [N+1][8]
    int every[kChainGroupMax];     // 0: nothing to do for this member
    int N, pad_;
};
hipError_t chain_gather_moments(hipStream_t st, const ChainGatherArgs& a, int K);

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
