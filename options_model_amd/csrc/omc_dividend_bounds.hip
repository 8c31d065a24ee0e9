// omc_dividend_bounds.hip -- Andersen-Broadie price bounds for a stock that pays discrete dividends: GBM and Heston,
// DESIGN.md section 29.
//
// The four sweeps that simulate fresh paths (bounds_lower_body, bounds_inner_body: omc_bounds_dev.h;
// bounds_sched_inner_body: omc_bounds_sched_dev.h; bounds_check_inner_body: omc_bounds_check_dev.h) with the dividend law
// of omc_dividend.hip as their Model, and the dividend generator that keeps the variance state of the outer paths.
// Every spot is the dividend generator's: the vanilla step of gbm_paths_body / heston_pair_step<SCHEME> at the drift rate
// r - q from the pair's blocks of normals, and on a dividend step, after it, s = fmaxf(fmaf(s, mul, -cash), 0) for both
// partners (include/omc.h, "dividends").
// The step of a date depends on the date, and the sweeps hand step() neither the date nor the pair.  So the law carries
// them: a Start says where in the dividend table a path of its date stands (DivStart: the next entry and how many of the
// path's own steps away it is, in one word), a lane keeps that word in its Spots and counts it down.  Inside the inner
// sweeps the lanes of a wave sit at different dates -- a lane is refilled when its pair has stopped -- so the generator's
// scalar "next entry" does not carry over: a step takes 1 off the lane's word and tests its low half, then one ballot
// over the lanes that execute the step (inside the sweeps' divergent code the ballot covers exactly those), and a scalar
// branch: where no live lane has a dividend the vanilla step runs and nothing else -- no fma, no max, no table read.  A
// lane that has one loads its 16-byte entry from global memory, which also says how far the following entry is.  In the
// lower sweep every lane of a wave is at the same date: there the word is read through readfirstlane, the test and the
// entry's load are scalar.
#include "omc_dividend_bounds.h"

#include "omc_bounds_check_dev.h"
#include "omc_bounds_dev.h"
#include "omc_bounds_sched_dev.h"
#include "omc_paths_dev.h"

namespace omc {

// what the dividend kernels take by value: the common arguments (v.a, v.b: the GBM step constants at the drift rate), the
// Heston law's float32 constants at the drift rate, and the dividend tables
struct DividendBoundsArgs {
    BoundsArgs v;
    HestonC hc;
    float v0;               // (float)v0: the variance every lower pair starts at
    const float* Vo;        // [N+1][n_outer] variance state of the outer paths (Heston)
    const DivEntry* tab;    // the dividend steps in step order + the closing entry; pad = steps to the next entry
    const DivStart* first;  // [N+1] where a path that starts at date t stands in tab
};

// the dividend path law (the Model of omc_bounds_dev.h); MODEL 0 GBM, 1 / 2 Heston scheme 0 / 1; the policy sees the
// spot.  UNIFORM: every lane of a wave is at the same date (the lower sweep)
template <int MODEL, bool UNIFORM>
struct DividendBoundsModel {
    struct Start { float s, v; DivStart at; };
    struct Spots { float sa, sb, va, vb; DivStart at; };  // (GBM: va, vb are never read)
    using Normals = float[MODEL == 0 ? 4 : 8];            // four steps: one block of GBM, two of Heston
    const DividendBoundsArgs& g;
    __device__ __forceinline__ Start lower_start() const
    {
        return Start{g.v.s0, g.v0, (DivStart)__builtin_amdgcn_readfirstlane((int)g.first[0])};
    }
    // the outer state (S_t[i], V_t[i]) and the date's place in the table: one address each per wave, held as scalars
    __device__ __forceinline__ Start inner_start(int t, int64_t i) const
    {
        const size_t at = (size_t)t * g.v.n_outer + i;
        Start s0;
        s0.s = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(g.v.So[at])));
        if constexpr (MODEL == 0) s0.v = 0.0f;
        else s0.v = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(g.Vo[at])));
        s0.at = (DivStart)__builtin_amdgcn_readfirstlane((int)g.first[t]);
        return s0;
    }
    __device__ __forceinline__ void reset(Spots& s, const Start& s0) const
    {
        s.sa = s.sb = s0.s;
        s.va = s.vb = s0.v;
        s.at = s0.at;
    }
    // four steps of generator pair `pair`: its normals (GBM block blk; Heston blocks 2 blk and 2 blk + 1)
    __device__ __forceinline__ void draw(uint64_t pair, uint32_t blk, uint32_t stream, Normals& z) const
    {
        if constexpr (MODEL == 0) {
            normals4(pair, blk, stream, g.v.k0, g.v.k1, z);
        } else {
            normals4(pair, 2 * blk, stream, g.v.k0, g.v.k1, reinterpret_cast<float(&)[4]>(z[0]));
            normals4(pair, 2 * blk + 1, stream, g.v.k0, g.v.k1, reinterpret_cast<float(&)[4]>(z[4]));
        }
    }
    __device__ __forceinline__ void vanilla(Spots& s, const Normals& z, int u) const
    {
        if constexpr (MODEL == 0) {
            s.sa = s.sa * fast_exp2(__builtin_fmaf(g.v.b, z[u], g.v.a));
            s.sb = s.sb * fast_exp2(__builtin_fmaf(-g.v.b, z[u], g.v.a));
        } else {
            heston_pair_step<MODEL - 1>(g.hc, z[2 * u], z[2 * u + 1], s.sa, s.va, s.sb, s.vb);
        }
    }
    __device__ __forceinline__ void pay(Spots& s, const DivEntry& e) const
    {
        s.sa = __builtin_fmaxf(__builtin_fmaf(s.sa, e.mul, -e.cash), 0.0f);
        s.sb = __builtin_fmaxf(__builtin_fmaf(s.sb, e.mul, -e.cash), 0.0f);
    }
    __device__ __forceinline__ void step(Spots& s, const Normals& z, int u) const
    {
        vanilla(s, z, u);
        if constexpr (UNIFORM) {
            DivStart at = (DivStart)__builtin_amdgcn_readfirstlane((int)s.at) - 1u;
            if ((at & 0xffffu) == 0) {  // a scalar compare: the whole wave has the dividend
                const DivEntry e = g.tab[at >> 16];
                pay(s, e);
                at += 0x10000u + (uint32_t)e.pad;
            }
            s.at = at;
        } else {
            s.at -= 1u;
            const bool hit = (s.at & 0xffffu) == 0;
            if (__builtin_amdgcn_ballot_w64(hit) != 0) {  // (the vanilla step and nothing else where no live lane has one)
                if (hit) {
                    const DivEntry e = g.tab[s.at >> 16];
                    pay(s, e);
                    s.at += 0x10000u + (uint32_t)e.pad;
                }
            }
        }
    }
    __device__ __forceinline__ float index_a(const Spots& s) const { return s.sa; }
    __device__ __forceinline__ float index_b(const Spots& s) const { return s.sb; }
};

template <int MODEL>
__global__ __launch_bounds__(kBlock) void dividend_bounds_lower_kernel(DividendBoundsArgs g, int nblk)
{
    extern __shared__ uint4 sh_bt[];
    __shared__ double red[kNQ * kRedStride];
    bounds_lower_body(g.v, DividendBoundsModel<MODEL, true>{g}, nblk, sh_bt, red);
}

template <int MODEL>
__global__ __launch_bounds__(kBlock) void dividend_bounds_inner_kernel(DividendBoundsArgs g, int64_t i0, int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bounds_inner_body(g.v, DividendBoundsModel<MODEL, false>{g}, i0, ni, sh_bt);
}

// the inner sweep of an exercise schedule (omc_bounds_sched_dev.h) under the dividend law
template <int MODEL>
__global__ __launch_bounds__(kBlock) void dividend_bounds_sched_inner_kernel(DividendBoundsArgs g, BoundsSched sc, int64_t i0,
                                                                             int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bounds_sched_inner_body(g.v, sc, DividendBoundsModel<MODEL, false>{g}, i0, ni, sh_bt);
}

// the list-driven inner sweep of sub-optimality checking (omc_bounds_check_dev.h) under the dividend law
template <int MODEL>
__global__ __launch_bounds__(kBlock) void dividend_bounds_check_inner_kernel(DividendBoundsArgs g, BoundsCheck k, int64_t i0,
                                                                             int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bounds_check_inner_body(g.v, k, DividendBoundsModel<MODEL, false>{g}, i0, ni, sh_bt);
}

// ------------------------------------------------------------------ the generator that keeps the variance
// dividend_paths_kernel<SCHEME + 1, 1> with V beside S: the same counters, the same steps, the same spots
template <int SCHEME>
__global__ __launch_bounds__(kBlock) void dividend_paths_sv_kernel(PathArgs g, const DivEntry* __restrict__ tab,
                                                                   float* __restrict__ V)
{
    float* __restrict__ S = g.S;
    const int64_t ld = g.ld, P = g.P;
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= P) return;
    float s = g.s_init, sa = g.s_init, va = g.v_init, vb = g.v_init;
    int64_t at = p;
    S[at] = s;
    S[at + P] = sa;
    V[at] = va;
    V[at + P] = vb;
    const int nblk = (g.n_steps + 1) >> 1;
    DivEntry e = tab[0];  // the next dividend step: the same for every lane
    int next = 1;
    int t = 0;
    for (int blk = 0; blk < nblk; ++blk) {
        float z[4];
        normals4(g.pair_offset + (uint64_t)p, (uint32_t)blk, g.stream, g.k0, g.k1, z);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (++t > g.n_steps) break;
            at += ld;
            heston_pair_step<SCHEME>(g.hc, z[2 * i], z[2 * i + 1], s, va, sa, vb);
            if (t == e.step) {
                s = __builtin_fmaxf(__builtin_fmaf(s, e.mul, -e.cash), 0.0f);
                sa = __builtin_fmaxf(__builtin_fmaf(sa, e.mul, -e.cash), 0.0f);
                e = tab[next++];
            }
            S[at] = s;
            S[at + P] = sa;
            V[at] = va;
            V[at + P] = vb;
        }
    }
}

// ------------------------------------------------------------------ launchers
hipError_t launch_dividend_paths_sv(hipStream_t st, const DividendGen& a, float* V)
{
    const PathSpec& s = a.paths;
    const int64_t P = s.n_paths / 2;
    if (P <= 0) return hipSuccess;
    if (s.model != 1 || s.scheme < 0 || s.scheme > 3) return hipErrorInvalidValue;
    const PathArgs g = make_path_args(s, P);
    const dim3 grid((unsigned)((P + kBlock - 1) / kBlock)), block(kBlock);
    for_scheme(s.scheme, [&](auto sc) {
        hipLaunchKernelGGL((dividend_paths_sv_kernel<decltype(sc)::value>), grid, block, 0, st, g, a.tab, V);
    });
    return hipGetLastError();
}

// the kernels' model number, or -1 for a law that has none
static int dividend_bounds_model(const DividendBoundsLaw& l)
{
    if (l.model == 0) return 0;
    return l.model == 1 && (l.scheme == 0 || l.scheme == 1) ? l.scheme + 1 : -1;
}

static DividendBoundsArgs dividend_bounds_args(const BoundsArgs& a, const DividendBoundsLaw& l)
{
    DividendBoundsArgs g{};
    g.v = a;
    if (l.model == 0) gbm_step_constants(l.drift_rate, l.sigma, l.T, a.N, &g.v.a, &g.v.b);
    else g.hc = make_heston(l.drift_rate, l.T, a.N, l.kappa, l.theta, l.xi, l.rho);
    g.v0 = (float)l.v0;
    g.Vo = l.Vo;
    g.tab = l.tab;
    g.first = l.first;
    return g;
}

// the inner sweeps' grid: four item waves per workgroup, at most 2048 workgroups (bounds_inner's)
static unsigned inner_grid(int64_t items)
{
    const int64_t nb = (items + 3) / 4;
    return (unsigned)(nb > 2048 ? 2048 : nb);
}

hipError_t dividend_bounds_lower(hipStream_t st, const BoundsArgs& a, const DividendBoundsLaw& l, double* result)
{
    const int mo = dividend_bounds_model(l);
    if (mo < 0) return hipErrorInvalidValue;
    const DividendBoundsArgs g = dividend_bounds_args(a, l);
    const int nblk = (int)bounds_lower_blocks(a);  // the vanilla sweep's grid
    const size_t lds = sizeof(uint4) * (size_t)(a.N + 1);
    for_int<0, 1, 2>(mo, [&](auto model) {
        hipLaunchKernelGGL((dividend_bounds_lower_kernel<decltype(model)::value>), dim3(nblk), dim3(kBlock), lds, st, g, nblk);
    });
    return lsm_finalize(st, a.part, nullptr, result, nblk, 0);
}

hipError_t dividend_bounds_inner(hipStream_t st, const BoundsArgs& a, const DividendBoundsLaw& l, int64_t i0, int64_t ni)
{
    const int mo = dividend_bounds_model(l);
    if (mo < 0) return hipErrorInvalidValue;
    const DividendBoundsArgs g = dividend_bounds_args(a, l);
    const size_t lds = sizeof(uint4) * (size_t)(a.N + 1);
    for_int<0, 1, 2>(mo, [&](auto model) {
        hipLaunchKernelGGL((dividend_bounds_inner_kernel<decltype(model)::value>), dim3(inner_grid(ni * a.N)), dim3(kBlock),
                           lds, st, g, i0, ni);
    });
    return hipGetLastError();
}

hipError_t dividend_bounds_sched_inner(hipStream_t st, const BoundsArgs& a, const DividendBoundsLaw& l, const BoundsSched& sc,
                                       int64_t i0, int64_t ni)
{
    const int mo = dividend_bounds_model(l);
    if (mo < 0 || !bounds_schedule_ok(sc, a.N)) return hipErrorInvalidValue;
    const DividendBoundsArgs g = dividend_bounds_args(a, l);
    const size_t lds = sizeof(uint4) * (size_t)(a.N + 1);
    for_int<0, 1, 2>(mo, [&](auto model) {
        hipLaunchKernelGGL((dividend_bounds_sched_inner_kernel<decltype(model)::value>), dim3(inner_grid(ni * sc.J)),
                           dim3(kBlock), lds, st, g, sc, i0, ni);
    });
    return hipGetLastError();
}

hipError_t dividend_bounds_check_inner(hipStream_t st, const BoundsArgs& a, const DividendBoundsLaw& l, const BoundsCheck& k,
                                       int64_t i0, int64_t ni)
{
    const int mo = dividend_bounds_model(l);
    if (mo < 0) return hipErrorInvalidValue;
    const DividendBoundsArgs g = dividend_bounds_args(a, l);
    const size_t lds = sizeof(uint4) * (size_t)(a.N + 1);
    // the dense sweep's grid: the kept items are a subset
    for_int<0, 1, 2>(mo, [&](auto model) {
        hipLaunchKernelGGL((dividend_bounds_check_inner_kernel<decltype(model)::value>), dim3(inner_grid(ni * a.N)),
                           dim3(kBlock), lds, st, g, k, i0, ni);
    });
    return hipGetLastError();
}

}  // namespace omc
