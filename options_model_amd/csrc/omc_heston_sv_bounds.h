// omc_heston_sv_bounds.h -- host interface of the Heston bound kernels whose policy sees the spot AND the variance state
// (omc_heston_sv_bounds.hip; the definitions are include/omc.h's).
#pragma once
#include "omc_heston_bounds.h"
#include "omc_runnerup_bounds.h"

namespace omc {

constexpr int kHestonSvMaxSteps = kRunnerupMaxSteps;  // dates whose policy rows (64 bytes each) live in LDS: section 18.1's cap

// the Heston law of the call, the two-regressor policy and the scale of its second regressor.  Of BoundsArgs the kernels
// read neither betas nor tab.
struct HestonSvLaw {
    DiffusionLaw h;     // model 1, scheme 0 or 1
    const double* pol;  // [N+1][8] device
    double inv_vbar;    // 1 / max(v0, theta): w = fma(V, inv_vbar, -1)
};

// the Longstaff-Schwartz fit on the paths of launch_heston_paths_sv: S, V in, policy rows 1 .. N-1 out
struct HestonSvFit {
    const float* S;  // [N+1][ld] spots of the fitting paths
    const float* V;  // [N+1][ld] their variance state
    int64_t ld, M;
    int N, is_put;
    double K, invK, inv_vbar;
    const double* D;  // [N+1] exp(-r dt k)
    float* x_ex;      // [M] the spot at the path's exercise date
    int32_t* tex;     // [M] that date
    double* part;     // [kRunnerupSlots][kRunnerupFitBlocks] per-workgroup partial sums of one date
    double* pol;      // [N+1][8]: rows 0 and N cleared, rows N-1 .. 1 fitted
};

hipError_t heston_sv_fit(hipStream_t st, const HestonSvFit& f);
// scheme 0 or 1 and at most kHestonSvMaxSteps dates, anything else is hipErrorInvalidValue
hipError_t heston_sv_lower(hipStream_t st, const BoundsArgs& a, const HestonSvLaw& l, double* result);
// Q^_t[i] for outer paths [i0, i0 + ni) and t = 0..N-1
hipError_t heston_sv_inner(hipStream_t st, const BoundsArgs& a, const HestonSvLaw& l, int64_t i0, int64_t ni);
hipError_t heston_sv_walk(hipStream_t st, const BoundsArgs& a, const HestonSvLaw& l, double* result);

}  // namespace omc
