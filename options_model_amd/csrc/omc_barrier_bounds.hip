// omc_barrier_bounds.hip -- Andersen-Broadie price bounds for knock-in / knock-out barrier options, discrete monitoring:
// GBM and Heston, DESIGN.md section 31.
//
// The four sweeps that simulate fresh paths (bounds_lower_body, bounds_inner_body: omc_bounds_dev.h;
// bounds_sched_inner_body: omc_bounds_sched_dev.h; bounds_check_inner_body: omc_bounds_check_dev.h) with the barrier law as
// their Model, the generator that keeps the outer paths' state, and the keep mask that takes a knock-out's dead items out
// of the list-driven sweep.
// Every spot is the barrier generator's (omc_barrier.hip): the vanilla step of gbm_paths_body / heston_pair_step<SCHEME> from
// the pair's blocks of normals, then the float32 test sg * s <= sthr on the REAL spot of either partner.  What the policy
// sees is the ENCODED index: the real spot where the option is live, barrier_dead_spot where it is not -- out of the money,
// so the exercise tables never fire on it.
// The knock state.  The generator keeps two bools per pair and selects per store (section 11.5: 16-bit registers and a
// select per flag).  Here a partner's state is one float32 register: m = min over the steps taken of sg * s, started at
// +inf (not hit) or -inf (hit at the start).  The flag is monotone, so "hit" is m <= sthr at any time: a step is a multiply
// and a v_min_f32, and the index is one compare (whose lane mask is inverted for a knock-out by a scalar xor, the kind being
// wave-uniform) and one select.
// A knocked-out partner stops -- kStops of omc_bounds_dev.h -- at the first exercise date at or after its hit step, at its
// index there, the dead spot, whose payoff is 0.  The inner sweeps mark exercise dates only; the lower sweep marks every
// date of the grid (a schedule reaches it as empty exercise tables), so under a schedule its Model tests the date (SCHED).
// A knock-in that has not hit keeps stepping and monitoring behind the dead spot.  An item of a knock-out that is dead at
// its start is never simulated: the list-driven sweep's list does not hold it (barrier_mark_kernel), the scheduled sweep
// starts none of its lanes (start_dead).
#include "omc_barrier_bounds.h"

#include "omc_bounds_law_dev.h"

namespace omc {

// what the barrier kernels take by value: the diffusion -- whose So is the REAL spots of the outer paths, the sweeps start
// from them and read So nowhere else -- and the contract
struct BarrierBoundsArgs {
    DiffusionArgs d;
    const int32_t* hit;  // [n_outer] first-hit steps of the outer paths
    float sg, sthr, dead;
    int knock_out;
    int every;  // the lower sweep under a schedule (SCHED): exercise dates are those with (N - d) % every == 0
};

// min(m, x) as ONE v_min_f32 (floor_at's reason, omc_paths_dev.h); a NaN x leaves m, as the generator's compare does
__device__ __forceinline__ float running_min(float m, float x)
{
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(m), "v"(x));
    return r;
}

// the barrier path law (the Model of omc_bounds_dev.h) on the diffusion MODEL 0 GBM, 1 / 2 Heston scheme 0 / 1.  SCHED: the
// sweep marks dates that are no exercise dates (the lower sweep of a scheduled game)
template <int MODEL, bool SCHED>
struct BarrierBoundsModel : DiffusionModel<MODEL> {
    using Base = DiffusionModel<MODEL>;
    using Args = BarrierBoundsArgs;
    using Normals = typename Base::Normals;
    static constexpr bool kStops = true;
    struct Start : Base::Start { float m; };        // +inf: not hit at the start, -inf: hit
    struct Spots : Base::Spots { float ma, mb; };   // min of sg * s over the start and the steps taken
    const Args& g;
    __device__ __forceinline__ BarrierBoundsModel(const Args& g) : Base{g.d}, g(g) {}
    static __device__ __forceinline__ const BoundsArgs& common(const Args& g) { return g.d.v; }
    __device__ __forceinline__ Start lower_start() const { return Start{Base::lower_start(), __builtin_inff()}; }
    // the outer state (S_t[i][, V_t[i]], hit(t, i)): one address per wave, held as scalars
    __device__ __forceinline__ Start inner_start(int t, int64_t i) const
    {
        const int h = __builtin_amdgcn_readfirstlane(g.hit[i]);
        return Start{Base::inner_start(t, i), h != 0 && h <= t ? -__builtin_inff() : __builtin_inff()};
    }
    __device__ __forceinline__ void reset(Spots& s, const Start& s0) const
    {
        Base::reset(s, s0);
        s.ma = s.mb = s0.m;
    }
    __device__ __forceinline__ void step(Spots& s, const Normals& z, int u) const
    {
        Base::step(s, z, u);
        s.ma = running_min(s.ma, g.sg * s.sa);
        s.mb = running_min(s.mb, g.sg * s.sb);
    }
    __device__ __forceinline__ bool hit(float m) const { return m <= g.sthr; }
    __device__ __forceinline__ bool ko() const { return g.knock_out != 0; }
    __device__ __forceinline__ float index_a(const Spots& s) const { return hit(s.ma) != ko() ? s.sa : g.dead; }
    __device__ __forceinline__ float index_b(const Spots& s) const { return hit(s.mb) != ko() ? s.sb : g.dead; }
    // (d is the same for every lane of the lower sweep: a scalar remainder; the date N is always an exercise date)
    __device__ __forceinline__ bool open(int d) const
    {
        if constexpr (SCHED) return (g.d.v.N - d) % g.every == 0;
        else return true;
    }
    __device__ __forceinline__ bool stopped_a(const Spots& s, int d) const { return ko() && hit(s.ma) && open(d); }
    __device__ __forceinline__ bool stopped_b(const Spots& s, int d) const { return ko() && hit(s.mb) && open(d); }
    __device__ __forceinline__ bool start_dead(const Start& s0) const { return ko() && hit(s0.m); }
};
template <int MODEL>
using BarrierModel = BarrierBoundsModel<MODEL, false>;
template <int MODEL>
using BarrierSchedLowerModel = BarrierBoundsModel<MODEL, true>;

// ------------------------------------------------------------------ the generator that keeps the outer state
// barrier_paths_body<MODEL, true, 0, 1, false>'s encoded matrix with the real spots, the variance (MODEL >= 1) and the
// first-hit steps beside it: the same counters, the same steps, the same test.  One pair per thread.
template <int MODEL>
__global__ __launch_bounds__(kBlock) void barrier_paths_state_kernel(PathArgs g, BarrierTest b, int start_hit,
                                                                     float* __restrict__ Sr, float* __restrict__ V,
                                                                     int32_t* __restrict__ hit)
{
    float* __restrict__ E = g.S;
    const int64_t ld = g.ld, P = g.P;
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= P) return;
    const bool ko = b.knock_out != 0;
    float s = g.s_init, sa = g.s_init, va = g.v_init, vb = g.v_init;
    int ha = start_hit ? -1 : 0, hb = ha;  // first-hit steps, 0 while not hit
    int64_t at = p;
    auto put = [&]() {
        E[at] = ((ha != 0) != ko) ? s : b.dead;
        E[at + P] = ((hb != 0) != ko) ? sa : b.dead;
        Sr[at] = s;
        Sr[at + P] = sa;
        if constexpr (MODEL != 0) {
            V[at] = va;
            V[at + P] = vb;
        }
    };
    put();
    constexpr int SPB = MODEL == 0 ? 4 : 2;  // steps per Philox block of normals
    const int nblk = (g.n_steps + SPB - 1) / SPB;
    int t = 0;
    for (int blk = 0; blk < nblk; ++blk) {
        float z[4];
        normals4(g.pair_offset + (uint64_t)p, (uint32_t)blk, g.stream, g.k0, g.k1, z);
#pragma unroll
        for (int i = 0; i < SPB; ++i) {
            if (++t > g.n_steps) break;
            at += ld;
            pair_step<MODEL>(g, z, i, s, va, sa, vb);
            ha = ha == 0 && b.sg * s <= b.sthr ? t : ha;
            hb = hb == 0 && b.sg * sa <= b.sthr ? t : hb;
            put();
        }
    }
    hit[p] = ha;
    hit[p + P] = hb;
}

// ------------------------------------------------------------------ the keep mask of a knock-out (k.mode 0)
// bounds_check_mark_body's outputs -- the mask [N][n_outer] and the kept items per (inner launch, date) -- with the rule
// "kept unless dead": one thread per (t, i)
__global__ __launch_bounds__(kBlock) void barrier_mark_kernel(int N, int64_t n_outer, const int32_t* __restrict__ hit,
                                                              int knock_out, BoundsCheck k)
{
    const int64_t n = (int64_t)N * n_outer;
    for (int64_t at = (int64_t)blockIdx.x * kBlock + threadIdx.x; at < n; at += (int64_t)gridDim.x * kBlock) {
        const int t = (int)(at / n_outer);
        const int64_t i = at - (int64_t)t * n_outer;
        const int h = hit[i];
        const bool keep = !(knock_out != 0 && h != 0 && h <= t);
        k.keep[at] = keep ? 1 : 0;
        // the kept items of (launch block, date): one atomic per wave where its lanes share the slot, else one per kept item
        const uint32_t slot = (uint32_t)((i / k.blk) * N + t);  // < n_outer N < 2^32
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot);
        const uint64_t live = __builtin_amdgcn_ballot_w64(true), kept = __builtin_amdgcn_ballot_w64(keep);
        if (__builtin_amdgcn_ballot_w64(slot != first) == 0) {
            const bool lead = __builtin_amdgcn_mbcnt_hi((uint32_t)(live >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)live, 0)) == 0;
            if (lead && kept) atomicAdd(k.per_date + first, (uint32_t)__popcll(kept));
        } else if (keep) {
            atomicAdd(k.per_date + slot, 1u);
        }
    }
}

// ------------------------------------------------------------------ launchers
BarrierTest barrier_test(double K, int is_put, double H, int up, int knock_in)
{
    const float thr = barrier_threshold(H, up);
    return {up ? -1.0f : 1.0f, up ? -thr : thr, barrier_dead_spot(K, is_put), knock_in ? 0 : 1};
}

hipError_t launch_barrier_paths_state(hipStream_t st, const BarrierStateGen& a)
{
    const PathSpec& s = a.paths;
    const int64_t P = s.n_paths / 2;
    if (P <= 0) return hipSuccess;
    const int mo = s.model == 0 ? 0 : s.model == 1 && (s.scheme == 0 || s.scheme == 1) ? s.scheme + 1 : -1;
    if (mo < 0 || (mo != 0 && !a.V)) return hipErrorInvalidValue;
    const PathArgs g = make_path_args(s, P);
    const dim3 grid((unsigned)((P + kBlock - 1) / kBlock)), block(kBlock);
    for_int<0, 1, 2>(mo, [&](auto model) {
        hipLaunchKernelGGL((barrier_paths_state_kernel<decltype(model)::value>), grid, block, 0, st, g, a.test, a.start_hit, a.Sr,
                           a.V, a.hit);
    });
    return hipGetLastError();
}

static BarrierBoundsArgs barrier_args(const BoundsArgs& a, const BarrierBoundsLaw& l)
{
    BarrierBoundsArgs g{diffusion_args(a, l.d), l.hit, l.test.sg, l.test.sthr, l.test.dead, l.test.knock_out, l.every};
    g.d.v.So = l.Sr;  // the sweeps start from the real spot; the encoded a.So is the walk's and the keep mask's
    return g;
}

hipError_t bounds_lower(hipStream_t st, const BoundsArgs& a, const BarrierBoundsLaw& l, double* result)
{
    if (l.every >= 2)
        return launch_bounds_lower<BarrierSchedLowerModel, 0, 1, 2>(st, diffusion_model(l.d), a, barrier_args(a, l), result);
    return launch_bounds_lower<BarrierModel, 0, 1, 2>(st, diffusion_model(l.d), a, barrier_args(a, l), result);
}

hipError_t bounds_inner(hipStream_t st, const BoundsArgs& a, const BarrierBoundsLaw& l, int64_t i0, int64_t ni)
{
    return launch_bounds_inner<BarrierModel, 0, 1, 2>(st, diffusion_model(l.d), a, barrier_args(a, l), i0, ni);
}

hipError_t bounds_sched_inner(hipStream_t st, const BoundsArgs& a, const BarrierBoundsLaw& l, const BoundsSched& sc, int64_t i0,
                              int64_t ni)
{
    return launch_bounds_sched_inner<BarrierModel, 0, 1, 2>(st, diffusion_model(l.d), a, barrier_args(a, l), sc, i0, ni);
}

hipError_t bounds_check_inner(hipStream_t st, const BoundsArgs& a, const BarrierBoundsLaw& l, const BoundsCheck& k, int64_t i0,
                              int64_t ni)
{
    return launch_bounds_check_inner<BarrierModel, 0, 1, 2>(st, diffusion_model(l.d), a, barrier_args(a, l), k, i0, ni);
}

hipError_t barrier_bounds_mark(hipStream_t st, const BoundsArgs& a, const BarrierBoundsLaw& l, const BoundsCheck& k)
{
    const int64_t n = (int64_t)a.N * a.n_outer;
    const int64_t nb = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(barrier_mark_kernel, dim3((unsigned)(nb > 2048 ? 2048 : nb)), dim3(kBlock), 0, st, a.N, a.n_outer, l.hit,
                       l.test.knock_out, k);
    return hipGetLastError();
}

}  // namespace omc
