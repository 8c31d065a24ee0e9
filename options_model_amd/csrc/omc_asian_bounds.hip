// omc_asian_bounds.hip -- Andersen-Broadie price bounds of the running-average (Asian) index kinds with a policy that sees
// the average X AND the current basket value B, the other half of the Markov state (the definitions
// are include/omc.h's).
//
//   fit     classic Longstaff-Schwartz on the generator's kept index and asset matrices: one launch per date t = N-1 .. 1
//           that applies the rule of date t+1 to the path state (x_ex, tex) and leaves the 27 sums of date t's regression
//           per workgroup, and section 18's one-workgroup solve (runnerup_fit_solve: the LDL' is not restated).
//   lower   omc_basket_bounds.hip's Asian lower sweep with the two-regressor stop.
//   inner   the hot path, that file's Asian inner simulations with the two-regressor stop.
//   walk    the outer walk with the two-regressor stop on (Xo, B from the outer asset matrices).
// The bodies are omc_bounds2_dev.h's, instantiated with the path law of omc_asian_dev.h; both regressors are scaled by 1/K.
// Every spot and every average is the generator's, the sums are float64 in a fixed order: identical calls return identical
// bits.  D is a template parameter and the law comes by value: nothing is indexed at run time (no scratch).
#include "omc_asian_bounds.h"

#include "omc_asian_dev.h"

namespace omc {

template <int D>
__global__ __launch_bounds__(kBlock) void asian2_lower_kernel(RunnerupArgs g, int nblk)
{
    extern __shared__ double sh_pol[];
    __shared__ double red[kNQ * kRedStride];
    bounds2_lower_body(g.g.v, AsianModel<D>{g.g}, g.pol, g.g.v.invK, nblk, sh_pol, red);
}

template <int D>
__global__ __launch_bounds__(kBlock) void asian2_inner_kernel(RunnerupArgs g, int64_t i0, int64_t ni)
{
    extern __shared__ double sh_pol[];
    bounds2_inner_body(g.g.v, AsianModel<D>{g.g}, g.pol, g.g.v.invK, i0, ni, sh_pol);
}

template <int D>
__global__ __launch_bounds__(kBlock) void asian2_walk_kernel(RunnerupArgs g, int nblk)
{
    __shared__ double red[kNQ * kRedStride];
    bounds2_walk_body(g.g.v, AsianModel<D>{g.g}, g.pol, g.g.v.invK, nblk, red);
}

// the (x, y) of a fitting path: column j, row t of the index matrix, and B_t from the asset matrices
template <int D>
struct AsianStored {
    BasketLaw law;
    const float* __restrict__ S;
    const float* __restrict__ A;
    size_t astride;  // one asset's matrix
    __device__ __forceinline__ Pair2 operator()(size_t at) const
    {
        float s[D];
#pragma unroll
        for (int k = 0; k < D; ++k) s[k] = A[(size_t)k * astride + at];
        return {S[at], basket_index<OMC_BASKET_ARITHMETIC, D>(law, s)};
    }
};

template <int D>
__global__ __launch_bounds__(kBlock) void asian2_fit_sums_kernel(Fit2 f, BasketLaw law, const float* S, const float* A, int t,
                                                                 int nblk)
{
    __shared__ double red[kNQ * kRedStride];
    fit2_sums_body(f, AsianStored<D>{law, S, A, (size_t)(f.N + 1) * (size_t)f.ld}, t, nblk, red);
}

// ------------------------------------------------------------------ launchers
static bool asian2_ok(const RunnerupArgs& a)
{
    return a.g.d >= 1 && a.g.d <= kBasketMax && a.g.v.N <= kRunnerupMaxSteps && basket_kind_is_asian(a.g.law.kind) && a.g.Co;
}

hipError_t asian2_fit(hipStream_t st, const AsianFit& f)
{
    if (f.d < 1 || f.d > kBasketMax) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(f.pol, 0, sizeof(double) * kRunnerupCols * (size_t)(f.N + 1), st);
    if (e != hipSuccess) return e;
    const Fit2 g{f.ld, f.M, f.N, f.is_put, f.K, f.invK, f.invK, f.D, f.x_ex, f.tex, f.part, f.pol};
    int64_t nb = (f.M + kBlock - 1) / kBlock;
    const int nblk = (int)(nb < kRunnerupFitBlocks ? nb : kRunnerupFitBlocks);
    for (int t = f.N - 1; t >= 1; --t) {
        for_assets(f.d, [&](auto d) {
            hipLaunchKernelGGL((asian2_fit_sums_kernel<d()>), dim3(nblk), dim3(kBlock), 0, st, g, f.law, f.S, f.A, t, nblk);
        });
        e = runnerup_fit_solve(st, f.part, nblk, f.pol + (size_t)t * kRunnerupCols);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

static size_t asian2_policy_lds(const RunnerupArgs& a) { return sizeof(double) * kRunnerupCols * (size_t)(a.g.v.N + 1); }

hipError_t asian2_lower(hipStream_t st, const RunnerupArgs& a, double* result)
{
    if (!asian2_ok(a)) return hipErrorInvalidValue;
    const int nblk = (int)bounds_lower_blocks(a.g.v);  // the vanilla sweep's grid
    for_assets(a.g.d, [&](auto d) {
        hipLaunchKernelGGL((asian2_lower_kernel<d()>), dim3(nblk), dim3(kBlock), asian2_policy_lds(a), st, a, nblk);
    });
    return lsm_finalize(st, a.g.v.part, nullptr, result, nblk, 0);
}

hipError_t asian2_inner(hipStream_t st, const RunnerupArgs& a, int64_t i0, int64_t ni)
{
    if (!asian2_ok(a)) return hipErrorInvalidValue;
    const unsigned nb = bounds_inner_grid(ni * a.g.v.N);
    for_assets(a.g.d, [&](auto d) {
        hipLaunchKernelGGL((asian2_inner_kernel<d()>), dim3(nb), dim3(kBlock), asian2_policy_lds(a), st, a, i0, ni);
    });
    return hipGetLastError();
}

hipError_t asian2_walk(hipStream_t st, const RunnerupArgs& a, double* result)
{
    if (!asian2_ok(a)) return hipErrorInvalidValue;
    const int nblk = (int)bounds_walk_blocks(a.g.v);
    for_assets(a.g.d, [&](auto d) {
        hipLaunchKernelGGL((asian2_walk_kernel<d()>), dim3(nblk), dim3(kBlock), 0, st, a, nblk);
    });
    return lsm_finalize(st, a.g.v.part, nullptr, result, nblk, 0);
}

}  // namespace omc
