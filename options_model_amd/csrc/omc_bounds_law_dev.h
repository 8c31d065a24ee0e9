// omc_bounds_law_dev.h -- what the bound kernels of the one-asset path laws share around the sweep bodies (DESIGN.md section
// 30): the diffusion every such law steps with, the four __global__ wrappers of the sweeps that simulate fresh paths, and
// their host launchers.
//
//   DiffusionArgs    what a diffusion's kernels take by value; a law with more to say nests it first in its own block
//   DiffusionModel   Start, Spots, Normals, lower_start, inner_start, reset, draw and the vanilla pair step of GBM (MODEL 0)
//                    and Heston scheme 0 / 1 (MODEL 1 / 2): the generator's counters and steps.  A law derives its Model
//                    (omc_bounds_dev.h) from it and writes only what is its own, as a rule its step.
//   kernels          bounds_lower_kernel<Model>, bounds_inner_kernel<Model>, bounds_sched_inner_kernel<Model>,
//                    bounds_check_inner_kernel<Model>: the LDS and the body.  A Model names its argument block (Args), is
//                    built from one, and hands the body the BoundsArgs inside (common).
//   launchers        launch_bounds_lower / _inner / _sched_inner / _check_inner: the model number as a template argument
//                    (omc_dispatch.h), the grid and LDS of omc_bounds.h, the launch, and the lower sweep's finalize.
// Each law's .hip instantiates its own kernels through the launchers.
#pragma once
#include "omc_bounds_check_dev.h"
#include "omc_bounds_dev.h"
#include "omc_bounds_sched_dev.h"
#include "omc_dispatch.h"
#include "omc_paths_dev.h"

namespace omc {

// the common arguments (v.a, v.b: the GBM step constants at the drift rate) and the Heston law's float32 constants at the
// drift rate.  The kernels read their arguments by offset: a block that nests this one keeps it first.
struct DiffusionArgs {
    BoundsArgs v;
    HestonC hc;
    float v0;         // (float)v0: the variance every lower pair starts at
    const float* Vo;  // [N+1][n_outer] variance state of the outer paths (Heston)
};

template <int MODEL>
struct DiffusionModel {
    struct Start { float s, v; };
    struct Spots { float sa, sb, va, vb; };  // (GBM: va, vb are never read)
    using Normals = float[MODEL == 0 ? 4 : 8];  // four steps: one block of GBM, two of Heston
    using Args = DiffusionArgs;
    const DiffusionArgs& d;
    static __device__ __forceinline__ const BoundsArgs& common(const DiffusionArgs& d) { return d.v; }
    __device__ __forceinline__ Start lower_start() const { return Start{d.v.s0, d.v0}; }
    // the outer state (S_t[i], V_t[i]): one address per wave, held as scalars
    __device__ __forceinline__ Start inner_start(int t, int64_t i) const
    {
        const size_t at = (size_t)t * d.v.n_outer + i;
        Start s0;
        s0.s = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(d.v.So[at])));
        if constexpr (MODEL == 0) s0.v = 0.0f;
        else s0.v = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(d.Vo[at])));
        return s0;
    }
    __device__ __forceinline__ void reset(Spots& s, const Start& s0) const
    {
        s.sa = s.sb = s0.s;
        s.va = s.vb = s0.v;
    }
    // four steps of generator pair `pair`: GBM block blk; Heston blocks 2 blk and 2 blk + 1 (one Philox block per two steps)
    __device__ __forceinline__ void draw(uint64_t pair, uint32_t blk, uint32_t stream, Normals& z) const
    {
        if constexpr (MODEL == 0) {
            normals4(pair, blk, stream, d.v.k0, d.v.k1, z);
        } else {
            normals4(pair, 2 * blk, stream, d.v.k0, d.v.k1, reinterpret_cast<float(&)[4]>(z[0]));
            normals4(pair, 2 * blk + 1, stream, d.v.k0, d.v.k1, reinterpret_cast<float(&)[4]>(z[4]));
        }
    }
    // the vanilla step of both partners with step u of the block
    __device__ __forceinline__ void step(Spots& s, const Normals& z, int u) const
    {
        if constexpr (MODEL == 0) {
            s.sa = s.sa * fast_exp2(__builtin_fmaf(d.v.b, z[u], d.v.a));
            s.sb = s.sb * fast_exp2(__builtin_fmaf(-d.v.b, z[u], d.v.a));
        } else {
            heston_pair_step<MODEL - 1>(d.hc, z[2 * u], z[2 * u + 1], s.sa, s.va, s.sb, s.vb);
        }
    }
    __device__ __forceinline__ float index_a(const Spots& s) const { return s.sa; }
    __device__ __forceinline__ float index_b(const Spots& s) const { return s.sb; }
};

// ------------------------------------------------------------------ the four sweeps that simulate fresh paths
template <class Model>
__global__ __launch_bounds__(kBlock) void bounds_lower_kernel(typename Model::Args g, int nblk)
{
    extern __shared__ uint4 sh_bt[];
    __shared__ double red[kNQ * kRedStride];
    bounds_lower_body(Model::common(g), Model{g}, nblk, sh_bt, red);
}

template <class Model>
__global__ __launch_bounds__(kBlock) void bounds_inner_kernel(typename Model::Args g, int64_t i0, int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bounds_inner_body(Model::common(g), Model{g}, i0, ni, sh_bt);
}

// the inner sweep of an exercise schedule (omc_bounds_sched_dev.h)
template <class Model>
__global__ __launch_bounds__(kBlock) void bounds_sched_inner_kernel(typename Model::Args g, BoundsSched sc, int64_t i0, int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bounds_sched_inner_body(Model::common(g), sc, Model{g}, i0, ni, sh_bt);
}

// the list-driven inner sweep of sub-optimality checking (omc_bounds_check_dev.h)
template <class Model>
__global__ __launch_bounds__(kBlock) void bounds_check_inner_kernel(typename Model::Args g, BoundsCheck k, int64_t i0, int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bounds_check_inner_body(Model::common(g), k, Model{g}, i0, ni, sh_bt);
}

// ------------------------------------------------------------------ host side
inline DiffusionArgs diffusion_args(const BoundsArgs& a, const DiffusionLaw& l)
{
    DiffusionArgs d{};
    d.v = a;
    if (l.model == 0) gbm_step_constants(l.drift_rate, l.sigma, l.T, a.N, &d.v.a, &d.v.b);
    else d.hc = make_heston(l.drift_rate, l.T, a.N, l.kappa, l.theta, l.xi, l.rho);
    d.v0 = (float)l.v0;
    d.Vo = l.Vo;
    return d;
}

// One launcher per sweep: Model<MODELS>... are the instantiations the law has, mo picks one (diffusion_model; a number that
// is not listed, -1 among them, is hipErrorInvalidValue), a the call's common arguments, g the law's block built from them.
template <int... MODELS>
inline bool bounds_model_listed(int mo)
{
    return ((mo == MODELS) || ...);
}

template <template <int> class Model, int... MODELS, class Args>
hipError_t launch_bounds_lower(hipStream_t st, int mo, const BoundsArgs& a, const Args& g, double* result)
{
    if (!bounds_model_listed<MODELS...>(mo)) return hipErrorInvalidValue;
    const int nblk = (int)bounds_lower_blocks(a);
    for_int<MODELS...>(mo, [&](auto model) {
        hipLaunchKernelGGL((bounds_lower_kernel<Model<decltype(model)::value>>), dim3(nblk), dim3(kBlock), bounds_table_lds(a.N),
                           st, g, nblk);
    });
    return lsm_finalize(st, a.part, nullptr, result, nblk, 0);
}

template <template <int> class Model, int... MODELS, class Args>
hipError_t launch_bounds_inner(hipStream_t st, int mo, const BoundsArgs& a, const Args& g, int64_t i0, int64_t ni)
{
    if (!bounds_model_listed<MODELS...>(mo)) return hipErrorInvalidValue;
    for_int<MODELS...>(mo, [&](auto model) {
        hipLaunchKernelGGL((bounds_inner_kernel<Model<decltype(model)::value>>), dim3(bounds_inner_grid(ni * a.N)), dim3(kBlock),
                           bounds_table_lds(a.N), st, g, i0, ni);
    });
    return hipGetLastError();
}

template <template <int> class Model, int... MODELS, class Args>
hipError_t launch_bounds_sched_inner(hipStream_t st, int mo, const BoundsArgs& a, const Args& g, const BoundsSched& sc, int64_t i0,
                                     int64_t ni)
{
    if (!bounds_model_listed<MODELS...>(mo) || !bounds_schedule_ok(sc, a.N)) return hipErrorInvalidValue;
    for_int<MODELS...>(mo, [&](auto model) {
        hipLaunchKernelGGL((bounds_sched_inner_kernel<Model<decltype(model)::value>>), dim3(bounds_inner_grid(ni * sc.J)),
                           dim3(kBlock), bounds_table_lds(a.N), st, g, sc, i0, ni);
    });
    return hipGetLastError();
}

// (the dense sweep's grid: the kept items are a subset, how many is known on the device alone)
template <template <int> class Model, int... MODELS, class Args>
hipError_t launch_bounds_check_inner(hipStream_t st, int mo, const BoundsArgs& a, const Args& g, const BoundsCheck& k, int64_t i0,
                                     int64_t ni)
{
    if (!bounds_model_listed<MODELS...>(mo)) return hipErrorInvalidValue;
    for_int<MODELS...>(mo, [&](auto model) {
        hipLaunchKernelGGL((bounds_check_inner_kernel<Model<decltype(model)::value>>), dim3(bounds_inner_grid(ni * a.N)),
                           dim3(kBlock), bounds_table_lds(a.N), st, g, k, i0, ni);
    });
    return hipGetLastError();
}

// The generators that keep the variance state V beside S (one pair per thread, Heston schemes 0 .. 3): the pair count, the
// grid, the argument block and the scheme; launch(scheme constant, grid, block, PathArgs) launches the law's kernel
template <class Launch>
hipError_t launch_paths_sv(const PathSpec& s, Launch&& launch)
{
    const int64_t P = s.n_paths / 2;
    if (P <= 0) return hipSuccess;
    if (s.model != 1 || s.scheme < 0 || s.scheme > 3) return hipErrorInvalidValue;
    const PathArgs g = make_path_args(s, P);
    const dim3 grid((unsigned)((P + kBlock - 1) / kBlock)), block(kBlock);
    for_scheme(s.scheme, [&](auto sc) { launch(sc, grid, block, g); });
    return hipGetLastError();
}

}  // namespace omc
