// omc_asian_bounds.h -- host interface of the bound kernels of the running-average (Asian) index kinds whose policy sees the
// average AND the current basket value (omc_asian_bounds.hip; the definitions are include/omc.h's).
// The policy table, its LDS rows, the 512-date cap, the sums and the solve are section 18's (omc_runnerup_bounds.h).
#pragma once
#include "omc_runnerup_bounds.h"

namespace omc {

// the Longstaff-Schwartz fit on the generator's paths: index and asset matrices in, policy rows 1 .. N-1 out
struct AsianFit {
    BasketLaw law;      // by value
    int d;              // assets, 1 .. kBasketMax
    const float* S;     // [N+1][ld] index matrix of the fitting paths (the average)
    const float* A;     // [d][N+1][ld] their asset matrices
    int64_t ld, M;
    int N, is_put;
    double K, invK;
    const double* D;    // [N+1] exp(-r dt k)
    float* x_ex;        // [M] the index at the path's exercise date
    int32_t* tex;       // [M] that date
    double* part;       // [kRunnerupSlots][kRunnerupFitBlocks] per-workgroup partial sums of one date
    double* pol;        // [N+1][8]: rows 0 and N cleared, rows N-1 .. 1 fitted
};

// RunnerupArgs: a.g with Co set, a.pol the policy rows
hipError_t asian2_fit(hipStream_t st, const AsianFit& f);
hipError_t asian2_lower(hipStream_t st, const RunnerupArgs& a, double* result);
// Q^_t[i] for outer paths [i0, i0 + ni) and t = 0..N-1
hipError_t asian2_inner(hipStream_t st, const RunnerupArgs& a, int64_t i0, int64_t ni);
hipError_t asian2_walk(hipStream_t st, const RunnerupArgs& a, double* result);

}  // namespace omc
