// omc_heston_sv_bounds.hip -- Andersen-Broadie price bounds under the Heston model with a policy that sees the spot X AND
// the variance state Y (the definitions are include/omc.h's).
//
//   fit     classic Longstaff-Schwartz on the (S, V) matrices of launch_heston_paths_sv: one launch per date t = N-1 .. 1
//           that applies the rule of date t+1 to the path state (x_ex, tex) and leaves the 27 sums of date t's regression
//           per workgroup, and section 18's one-workgroup solve (runnerup_fit_solve: the LDL' is not restated).
//   lower   omc_heston_bounds.hip's lower sweep with the two-regressor stop.
//   inner   the hot path, omc_heston_bounds.hip's inner simulations with the two-regressor stop.
//   walk    the outer walk with the two-regressor stop on (So, Vo).
// The bodies are omc_bounds2_dev.h's, instantiated for schemes 0 and 1.  The path law is the Heston bounds' own, the shared
// diffusion (DiffusionModel, omc_bounds_law_dev.h): normals4(pair, 2 blk) and normals4(pair, 2 blk + 1), four
// heston_pair_step<SCHEME> per draw, the item's (S_t[i], V_t[i]) read once per wave.  Y is
// the variance as heston_pair_step leaves it -- what the generator stores: scheme 0 floored at 0, scheme 1 unfloored --,
// scaled by 1 / max(v0, theta).  Every spot is the Heston generator's, the sums are float64 in a fixed order: identical
// calls return identical bits.  Nothing is indexed at run time (no scratch).
//
// omc_runnerup_bounds.hip still restates the two-regressor bodies for the basket generator; moving it onto
// omc_bounds2_dev.h is a refactor with its own bit-for-bit evidence and is not part of this file's change.
#include "omc_heston_sv_bounds.h"

#include "omc_bounds2_dev.h"
#include "omc_bounds_law_dev.h"

namespace omc {

// what the kernels take by value: the diffusion and the policy
struct HestonSvArgs {
    DiffusionArgs d;
    const double* pol;  // [N+1][8]
    double inv_vbar;
};

// the Heston path law; the policy sees (spot, variance) of either partner
template <int SCHEME>
struct HestonSvModel : DiffusionModel<SCHEME + 1> {
    using Base = DiffusionModel<SCHEME + 1>;
    using Spots = typename Base::Spots;
    __device__ __forceinline__ HestonSvModel(const HestonSvArgs& g) : Base{g.d} {}
    __device__ __forceinline__ Pair2 xy_a(const Spots& s) const { return {s.sa, s.va}; }
    __device__ __forceinline__ Pair2 xy_b(const Spots& s) const { return {s.sb, s.vb}; }
    __device__ __forceinline__ Pair2 xy_outer(int t, int64_t i) const
    {
        const size_t at = (size_t)t * this->d.v.n_outer + i;
        return {this->d.v.So[at], this->d.Vo[at]};
    }
};

template <int SCHEME>
__global__ __launch_bounds__(kBlock) void heston_sv_lower_kernel(HestonSvArgs g, int nblk)
{
    extern __shared__ double sh_pol[];
    __shared__ double red[kNQ * kRedStride];
    bounds2_lower_body(g.d.v, HestonSvModel<SCHEME>{g}, g.pol, g.inv_vbar, nblk, sh_pol, red);
}

template <int SCHEME>
__global__ __launch_bounds__(kBlock) void heston_sv_inner_kernel(HestonSvArgs g, int64_t i0, int64_t ni)
{
    extern __shared__ double sh_pol[];
    bounds2_inner_body(g.d.v, HestonSvModel<SCHEME>{g}, g.pol, g.inv_vbar, i0, ni, sh_pol);
}

// the walk reads stored states only: the scheme does not enter (the model's is any)
__global__ __launch_bounds__(kBlock) void heston_sv_walk_kernel(HestonSvArgs g, int nblk)
{
    __shared__ double red[kNQ * kRedStride];
    bounds2_walk_body(g.d.v, HestonSvModel<0>{g}, g.pol, g.inv_vbar, nblk, red);
}

// the (x, y) of a fitting path: column j, row t of S and V
struct HestonSvStored {
    const float* __restrict__ S;
    const float* __restrict__ V;
    __device__ __forceinline__ Pair2 operator()(size_t at) const { return {S[at], V[at]}; }
};

__global__ __launch_bounds__(kBlock) void heston_sv_fit_sums_kernel(Fit2 f, const float* S, const float* V, int t, int nblk)
{
    __shared__ double red[kNQ * kRedStride];
    fit2_sums_body(f, HestonSvStored{S, V}, t, nblk, red);
}

// ------------------------------------------------------------------ launchers
hipError_t heston_sv_fit(hipStream_t st, const HestonSvFit& f)
{
    hipError_t e = hipMemsetAsync(f.pol, 0, sizeof(double) * kRunnerupCols * (size_t)(f.N + 1), st);
    if (e != hipSuccess) return e;
    const Fit2 g{f.ld, f.M, f.N, f.is_put, f.K, f.invK, f.inv_vbar, f.D, f.x_ex, f.tex, f.part, f.pol};
    int64_t nb = (f.M + kBlock - 1) / kBlock;
    const int nblk = (int)(nb < kRunnerupFitBlocks ? nb : kRunnerupFitBlocks);
    for (int t = f.N - 1; t >= 1; --t) {
        hipLaunchKernelGGL(heston_sv_fit_sums_kernel, dim3(nblk), dim3(kBlock), 0, st, g, f.S, f.V, t, nblk);
        e = runnerup_fit_solve(st, f.part, nblk, f.pol + (size_t)t * kRunnerupCols);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

static bool sv_ok(const BoundsArgs& a, const HestonSvLaw& l)
{
    return diffusion_model(l.h) >= 1 && a.N <= kHestonSvMaxSteps;
}

static HestonSvArgs sv_args(const BoundsArgs& a, const HestonSvLaw& l) { return {diffusion_args(a, l.h), l.pol, l.inv_vbar}; }

static size_t sv_policy_lds(const BoundsArgs& a) { return sizeof(double) * kRunnerupCols * (size_t)(a.N + 1); }

hipError_t heston_sv_lower(hipStream_t st, const BoundsArgs& a, const HestonSvLaw& l, double* result)
{
    if (!sv_ok(a, l)) return hipErrorInvalidValue;
    const HestonSvArgs g = sv_args(a, l);
    const int nblk = (int)bounds_lower_blocks(a);  // the vanilla sweep's grid
    for_int<0, 1>(l.h.scheme, [&](auto sc) {
        hipLaunchKernelGGL((heston_sv_lower_kernel<decltype(sc)::value>), dim3(nblk), dim3(kBlock), sv_policy_lds(a), st, g, nblk);
    });
    return lsm_finalize(st, a.part, nullptr, result, nblk, 0);
}

hipError_t heston_sv_inner(hipStream_t st, const BoundsArgs& a, const HestonSvLaw& l, int64_t i0, int64_t ni)
{
    if (!sv_ok(a, l)) return hipErrorInvalidValue;
    const HestonSvArgs g = sv_args(a, l);
    for_int<0, 1>(l.h.scheme, [&](auto sc) {
        hipLaunchKernelGGL((heston_sv_inner_kernel<decltype(sc)::value>), dim3(bounds_inner_grid(ni * a.N)), dim3(kBlock),
                           sv_policy_lds(a), st, g, i0, ni);
    });
    return hipGetLastError();
}

hipError_t heston_sv_walk(hipStream_t st, const BoundsArgs& a, const HestonSvLaw& l, double* result)
{
    if (!sv_ok(a, l)) return hipErrorInvalidValue;
    const HestonSvArgs g = sv_args(a, l);
    const int nblk = (int)bounds_walk_blocks(a);
    hipLaunchKernelGGL(heston_sv_walk_kernel, dim3(nblk), dim3(kBlock), 0, st, g, nblk);
    return lsm_finalize(st, a.part, nullptr, result, nblk, 0);
}

}  // namespace omc
