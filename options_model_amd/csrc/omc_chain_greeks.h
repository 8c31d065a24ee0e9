// omc_chain_greeks.h -- host interface of the option chain's Greeks kernels (omc_chain_greeks.hip; internal to libomc.so):
// the frozen-policy pathwise Greeks of many strikes, sides and exercise schedules of one expiry from ONE path matrix
// (omc_price_american_chain_greeks).
#pragma once
#include "omc_chain.h"
#include "omc_greeks.h"

namespace omc {

// One entry of a group, read by the group's three launches from DEVICE memory (the slots of a whole call are uploaded once,
// in front of the generator).  An American entry's view is the matrix itself (every = 1, N = the fine N); a Bermudan
// entry's holds its scheduled rows (omc_chain.h) and every table below is stated on the view's rows.
struct ChainGreeksSlot {
    const float* S;       // the view's row 0
    int64_t ld;           // the view's leading dimension: every x the matrix's
    double* betas;        // [N+1][4] the fits on the view's rows: solved here from gmom, or the caller's
    const double* gmom;   // [N+1][8] the reduced moments of pass 1; null: the fits are given (no solve, sum_nitm = 0)
    const double* cK;     // [N+1] the fold table on the view's rows; null = full storage
    const double* D;      // [N]   D[j - 1] values an exercise at view row j (the discount table, or the schedule's d2)
    double* part;         // [kGreeksQ][nblk] the sweep's per-workgroup partials
    double* result;       // [kGreeksQ]
    double K;
    int N;                // the view's steps Nv
    int every;            // the schedule: view row j is fine step Nf - every (Nv - j); 1 = every date
};
static_assert(sizeof(ChainGreeksSlot) == 80, "ChainGreeksSlot is read by the device as laid out here");

constexpr int kChainGreeksMax = kChainGroupMax;  // entries per sweep launch at most (option "chain_greeks_k")

// what the members of a call share; `slots` is the device array of the launch's entries
struct ChainGreeksArgs {
    const ChainGreeksSlot* slots;
    int64_t cols, nblk;  // the matrix's columns swept and its column blocks (greeks_blocks of the MATRIX)
    int vec;             // greeks_vec of the MATRIX (S, ld, cols): never of a view
    int Nf;              // the fine steps
    int gbm, order;      // order: kChainGreeksBanded / kChainGreeksPlain
    double S0, r, sigma, T, h;
};
// Block order of the sweep's grid -- speed only, the bits do not depend on it.  Banded: the entries of a band of 8 column
// blocks are dispatched together, the entry advancing the linear index by 8 (blocks b and b + 8 are observed to share an
// XCD, hence its L2); plain: entry slowest, E sweeps back to back in one grid.
constexpr int kChainGreeksBanded = 0, kChainGreeksPlain = 1;

// the sweep for entries [first, first + E) of a.slots, all of ONE side and storage (folded: their cK set); E <= kChainGreeksMax;
// n_max: the longest member's view steps (the launch's LDS)
hipError_t chain_greeks_sweep(hipStream_t st, const ChainGreeksArgs& a, int first, int E, int is_put, bool folded, int n_max);
// betas = the fits of gmom for members [0, E) that carry moments: lsm_solve_betas' launch, the entry on grid.y
hipError_t chain_greeks_solve(hipStream_t st, const ChainGreeksArgs& a, int E, int n_max);
// lsm_greeks' finalize for members [0, E), the entry on grid.y
hipError_t chain_greeks_finalize(hipStream_t st, const ChainGreeksArgs& a, int E);

}  // namespace omc
