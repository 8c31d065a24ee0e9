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

#include "omc_bounds_law_dev.h"

namespace omc {

// what the dividend kernels take by value: the diffusion at the drift rate and the dividend tables
struct DividendBoundsArgs {
    DiffusionArgs d;
    const DivEntry* tab;    // the dividend steps in step order + the closing entry; pad = steps to the next entry
    const DivStart* first;  // [N+1] where a path that starts at date t stands in tab
};

// the dividend path law (the Model of omc_bounds_dev.h) on the diffusion MODEL 0 GBM, 1 / 2 Heston scheme 0 / 1; the
// policy sees the spot.  UNIFORM: every lane of a wave is at the same date (the lower sweep)
template <int MODEL, bool UNIFORM>
struct DividendBoundsModel : DiffusionModel<MODEL> {
    using Base = DiffusionModel<MODEL>;
    using Args = DividendBoundsArgs;
    using Normals = typename Base::Normals;
    struct Start : Base::Start { DivStart at; };
    struct Spots : Base::Spots { DivStart at; };
    const Args& g;
    __device__ __forceinline__ DividendBoundsModel(const Args& g) : Base{g.d}, g(g) {}
    static __device__ __forceinline__ const BoundsArgs& common(const Args& g) { return g.d.v; }
    // the date's place in the table: one address per wave, held as a scalar
    __device__ __forceinline__ Start lower_start() const
    {
        return Start{Base::lower_start(), (DivStart)__builtin_amdgcn_readfirstlane((int)g.first[0])};
    }
    __device__ __forceinline__ Start inner_start(int t, int64_t i) const
    {
        return Start{Base::inner_start(t, i), (DivStart)__builtin_amdgcn_readfirstlane((int)g.first[t])};
    }
    __device__ __forceinline__ void reset(Spots& s, const Start& s0) const
    {
        Base::reset(s, s0);
        s.at = s0.at;
    }
    __device__ __forceinline__ void pay(Spots& s, const DivEntry& e) const
    {
        s.sa = __builtin_fmaxf(__builtin_fmaf(s.sa, e.mul, -e.cash), 0.0f);
        s.sb = __builtin_fmaxf(__builtin_fmaf(s.sb, e.mul, -e.cash), 0.0f);
    }
    __device__ __forceinline__ void step(Spots& s, const Normals& z, int u) const
    {
        Base::step(s, z, u);
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
};
template <int MODEL>
using DividendLowerModel = DividendBoundsModel<MODEL, true>;
template <int MODEL>
using DividendInnerModel = DividendBoundsModel<MODEL, false>;

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
    return launch_paths_sv(a.paths, [&](auto sc, dim3 grid, dim3 block, const PathArgs& g) {
        hipLaunchKernelGGL((dividend_paths_sv_kernel<decltype(sc)::value>), grid, block, 0, st, g, a.tab, V);
    });
}

static DividendBoundsArgs dividend_args(const BoundsArgs& a, const DividendBoundsLaw& l)
{
    return {diffusion_args(a, l.d), l.tab, l.first};
}

hipError_t bounds_lower(hipStream_t st, const BoundsArgs& a, const DividendBoundsLaw& l, double* result)
{
    return launch_bounds_lower<DividendLowerModel, 0, 1, 2>(st, diffusion_model(l.d), a, dividend_args(a, l), result);
}

hipError_t bounds_inner(hipStream_t st, const BoundsArgs& a, const DividendBoundsLaw& l, int64_t i0, int64_t ni)
{
    return launch_bounds_inner<DividendInnerModel, 0, 1, 2>(st, diffusion_model(l.d), a, dividend_args(a, l), i0, ni);
}

hipError_t bounds_sched_inner(hipStream_t st, const BoundsArgs& a, const DividendBoundsLaw& l, const BoundsSched& sc, int64_t i0,
                              int64_t ni)
{
    return launch_bounds_sched_inner<DividendInnerModel, 0, 1, 2>(st, diffusion_model(l.d), a, dividend_args(a, l), sc, i0, ni);
}

hipError_t bounds_check_inner(hipStream_t st, const BoundsArgs& a, const DividendBoundsLaw& l, const BoundsCheck& k, int64_t i0,
                              int64_t ni)
{
    return launch_bounds_check_inner<DividendInnerModel, 0, 1, 2>(st, diffusion_model(l.d), a, dividend_args(a, l), k, i0, ni);
}

}  // namespace omc
