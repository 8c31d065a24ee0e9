// omc_basket_bounds.hip -- Andersen-Broadie price bounds on the index of D correlated GBM assets.
//
// The two sweeps of omc_bounds.hip that simulate paths, with D assets per partner: the same bodies (bounds_lower_body,
// bounds_inner_body: omc_bounds_dev.h) with the path law below -- except the D = 1 inner kernel, which keeps a restated body
// (see there).
//   lower   one thread per antithetic pair of fresh paths, both partners' D spots in registers, each partner stopped at the
//           first date the rule fires on its INDEX.
//   inner   the hot path: a wave per (outer path, date) item, a lane per antithetic inner pair, four steps per Philox
//           block per asset.  The item's D start spots are the outer ASSET spots A_k[t][i]: loaded once per item,
//           wave-uniform, kept in scalar registers.
// Every spot is the basket generator's (omc_basket.hip, include/omc.h), from the generator's own helpers
// (omc_basket_dev.h): asset k of pair g draws normals4(g + (k << 40)), the correlated normals accumulate with k ascending
// in one fmaf chain, the step is s *= exp2(fmaf(+-b_k, y_k, a_k)), the index is the rule of the kind.  The law and the
// kind come by value; D is a template parameter so that every loop over assets unrolls and no array is indexed at run
// time (no scratch: section 17.3).
// With D = 1 and w = 1 both kernels perform the vanilla kernels' operations in the vanilla order: the same bits.
// The outer walk, the exercise tables and the finalize are omc_bounds.hip's / omc_lsm.hip's, on the index matrix.
// The Asian kinds (section 23) run the same two bodies with the path law of omc_asian_dev.h.
#include "omc_asian_dev.h"
#include "omc_basket_bounds.h"
#include "omc_basket_dev.h"
#include "omc_bounds_check_dev.h"
#include "omc_bounds_dev.h"

namespace omc {

// the path law of D correlated GBM assets (the Model of omc_bounds_dev.h); the policy sees the index
template <int D>
struct BasketBoundsModel {
    struct Start { float v[D]; };
    struct Spots { float a[D], b[D]; };
    using Normals = float[D][4];
    const BasketBoundsArgs& g;
    __device__ __forceinline__ Start lower_start() const
    {
        Start s0;
#pragma unroll
        for (int k = 0; k < D; ++k) s0.v[k] = g.law.s0[k];
        return s0;
    }
    // the outer asset spots A_k[t][i]: one address per wave, held as scalars
    __device__ __forceinline__ Start inner_start(int t, int64_t i) const
    {
        const size_t astride = (size_t)(g.v.N + 1) * (size_t)g.v.n_outer;  // one asset's outer matrix
        Start s0;
#pragma unroll
        for (int k = 0; k < D; ++k)
            s0.v[k] = __int_as_float(
                __builtin_amdgcn_readfirstlane(__float_as_int(g.Ao[(size_t)k * astride + (size_t)t * g.v.n_outer + i])));
        return s0;
    }
    __device__ __forceinline__ void reset(Spots& s, const Start& s0) const
    {
#pragma unroll
        for (int k = 0; k < D; ++k) s.a[k] = s.b[k] = s0.v[k];
    }
    __device__ __forceinline__ void draw(uint64_t pair, uint32_t blk, uint32_t stream, Normals& y) const
    {
        basket_normals<D>(g.law, pair, blk, stream, g.v.k0, g.v.k1, y);
    }
    __device__ __forceinline__ void step(Spots& s, const Normals& y, int u) const { basket_step<D>(g.law, s.a, s.b, y, u); }
    __device__ __forceinline__ float index_a(const Spots& s) const { return basket_law_index<D>(g.law, s.a); }
    __device__ __forceinline__ float index_b(const Spots& s) const { return basket_law_index<D>(g.law, s.b); }
};

template <int D>
__global__ __launch_bounds__(kBlock) void basket_bounds_lower_kernel(BasketBoundsArgs g, int nblk)
{
    extern __shared__ uint4 sh_bt[];
    __shared__ double red[kNQ * kRedStride];
    bounds_lower_body(g.v, BasketBoundsModel<D>{g}, nblk, sh_bt, red);
}

template <int D>
__global__ __launch_bounds__(kBlock) void basket_bounds_inner_kernel(BasketBoundsArgs g, int64_t i0, int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bounds_inner_body(g.v, BasketBoundsModel<D>{g}, i0, ni, sh_bt);
}

// D = 1 keeps the body it had before the shared one, restated: through bounds_inner_body this one kernel measured 0.5 - 1.2 %
// slower on the upper phase (profiles/bounds_body_time.txt), beyond the run-to-run noise; its instruction
// stream is the earlier one.  A change to bounds_inner_body's refill must be made here too.
template <>
__global__ __launch_bounds__(kBlock) void basket_bounds_inner_kernel<1>(BasketBoundsArgs g, int64_t i0, int64_t ni)
{
    constexpr int D = 1;
    extern __shared__ uint4 sh_bt[];
    const BoundsArgs& a = g.v;
    const BasketLaw& c = g.law;
    bd_load_tables(a, sh_bt);
    const int N = a.N;
    const int lane = (int)(threadIdx.x & 63);
    const int64_t H = a.half_inner;
    const int64_t n_items = ni * N;
    const int64_t nwaves = (int64_t)gridDim.x * (kBlock / 64);
    const size_t astride = (size_t)(N + 1) * (size_t)a.n_outer;  // one asset's outer matrix
    unsigned long long steps = 0;
    for (int64_t item = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); item < n_items; item += nwaves) {
        const int t = (int)(item / ni);
        const int64_t i = i0 + (item - (int64_t)t * ni);
        float s0[D];  // the item's start spots: one address per wave, held as scalars
#pragma unroll
        for (int k = 0; k < D; ++k)
            s0[k] = __int_as_float(
                __builtin_amdgcn_readfirstlane(__float_as_int(g.Ao[(size_t)k * astride + (size_t)t * a.n_outer + i])));
        const uint64_t gbase = ((uint64_t)i * (uint64_t)(N + 1) + (uint64_t)t) * (uint64_t)H;
        int64_t j = lane, next = 64;  // this lane's pair; the item's first unstarted pair
        bool act = j < H;
        float sa[D], sb[D], xa = 0.0f, xb = 0.0f;
#pragma unroll
        for (int k = 0; k < D; ++k) sa[k] = sb[k] = s0[k];
        int k = 0, da = 0, db = 0;  // steps taken by the pair; stop dates of its partners (0 while live)
        double acc = 0.0;
        while (__builtin_amdgcn_ballot_w64(act)) {
            if (act) {
                float y[D][4];
                basket_normals<D>(c, gbase + (uint64_t)j, (uint32_t)(k >> 2), a.stream_inner, a.k0, a.k1, y);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (da == 0 || db == 0) {
                        ++k;
                        const int d = t + k;
                        basket_step<D>(c, sa, sb, y, u);
                        const float ia = basket_law_index<D>(c, sa), ib = basket_law_index<D>(c, sb);
                        const uint4 iv = sh_bt[d];
                        const bool ea = da == 0 && bd_stop(ia, d, iv, a);
                        const bool eb = db == 0 && bd_stop(ib, d, iv, a);
                        xa = ea ? ia : xa;
                        da = ea ? d : da;
                        xb = eb ? ib : xb;
                        db = eb ? d : db;
                    }
                }
            }
            const bool done = act && da != 0 && db != 0;
            const uint64_t m = __builtin_amdgcn_ballot_w64(done);
            if (done) {
                acc += bd_value(xa, da, a) + bd_value(xb, db, a);
                steps += (unsigned long long)(da - t) + (unsigned long long)(db - t);
                // the finished lanes take the next pairs in lane order (mbcnt: finished lanes below this one)
                j = next + (int64_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
                act = j < H;
#pragma unroll
                for (int q = 0; q < D; ++q) sa[q] = sb[q] = s0[q];
                k = da = db = 0;
            }
            next += __popcll(m);
        }
        const double q = wave_sum_f64(acc);
        if (lane == 0) a.q[(size_t)i * N + t] = q / (double)(2 * H);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) steps += __shfl_xor(steps, off, 64);
    if (lane == 0 && steps) atomicAdd(a.steps, steps);
}

// ------------------------------------------------------------------ the running-average (Asian) kinds, section 23
// the same two bodies with the path law of omc_asian_dev.h: the running state beside the spots, the step counter in Spots
template <int D>
__global__ __launch_bounds__(kBlock) void asian_bounds_lower_kernel(BasketBoundsArgs g, int nblk)
{
    extern __shared__ uint4 sh_bt[];
    __shared__ double red[kNQ * kRedStride];
    bounds_lower_body(g.v, AsianModel<D>{g}, nblk, sh_bt, red);
}

template <int D>
__global__ __launch_bounds__(kBlock) void asian_bounds_inner_kernel(BasketBoundsArgs g, int64_t i0, int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bounds_inner_body(g.v, AsianModel<D>{g}, i0, ni, sh_bt);
}

// ------------------------------------------------------------------ sub-optimality checking, section 27
// the list-driven sweep of omc_bounds_check_dev.h with both path laws (D = 1 too: bounds_inner_body's sums, the same bits)
template <int D>
__global__ __launch_bounds__(kBlock) void basket_bounds_check_inner_kernel(BasketBoundsArgs g, BoundsCheck k, int64_t i0,
                                                                           int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bounds_check_inner_body(g.v, k, BasketBoundsModel<D>{g}, i0, ni, sh_bt);
}

template <int D>
__global__ __launch_bounds__(kBlock) void asian_bounds_check_inner_kernel(BasketBoundsArgs g, BoundsCheck k, int64_t i0,
                                                                          int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bounds_check_inner_body(g.v, k, AsianModel<D>{g}, i0, ni, sh_bt);
}

// ------------------------------------------------------------------ launchers
hipError_t basket_bounds_lower(hipStream_t st, const BasketBoundsArgs& a, double* result)
{
    if (a.d < 1 || a.d > kBasketMax) return hipErrorInvalidValue;
    const int nblk = (int)bounds_lower_blocks(a.v);  // the vanilla sweep's grid
    if (basket_kind_is_asian(a.law.kind)) {
        for_assets(a.d, [&](auto d) {
            hipLaunchKernelGGL((asian_bounds_lower_kernel<d()>), dim3(nblk), dim3(kBlock), sizeof(uint4) * (size_t)(a.v.N + 1),
                               st, a, nblk);
        });
        return lsm_finalize(st, a.v.part, nullptr, result, nblk, 0);
    }
    for_assets(a.d, [&](auto d) {
        hipLaunchKernelGGL((basket_bounds_lower_kernel<d()>), dim3(nblk), dim3(kBlock), sizeof(uint4) * (size_t)(a.v.N + 1), st,
                           a, nblk);
    });
    return lsm_finalize(st, a.v.part, nullptr, result, nblk, 0);
}

hipError_t basket_bounds_inner(hipStream_t st, const BasketBoundsArgs& a, int64_t i0, int64_t ni)
{
    if (a.d < 1 || a.d > kBasketMax) return hipErrorInvalidValue;
    const unsigned g = bounds_inner_grid(ni * a.v.N);
    if (basket_kind_is_asian(a.law.kind)) {
        if (!a.Co) return hipErrorInvalidValue;
        for_assets(a.d, [&](auto d) {
            hipLaunchKernelGGL((asian_bounds_inner_kernel<d()>), dim3((unsigned)g), dim3(kBlock),
                               sizeof(uint4) * (size_t)(a.v.N + 1), st, a, i0, ni);
        });
        return hipGetLastError();
    }
    for_assets(a.d, [&](auto d) {
        hipLaunchKernelGGL((basket_bounds_inner_kernel<d()>), dim3((unsigned)g), dim3(kBlock),
                           sizeof(uint4) * (size_t)(a.v.N + 1), st, a, i0, ni);
    });
    return hipGetLastError();
}

hipError_t basket_bounds_check_inner(hipStream_t st, const BasketBoundsArgs& a, const BoundsCheck& k, int64_t i0, int64_t ni)
{
    if (a.d < 1 || a.d > kBasketMax) return hipErrorInvalidValue;
    const unsigned g = bounds_inner_grid(ni * a.v.N);  // the dense sweep's grid: the kept items are a subset
    if (basket_kind_is_asian(a.law.kind)) {
        if (!a.Co) return hipErrorInvalidValue;
        for_assets(a.d, [&](auto d) {
            hipLaunchKernelGGL((asian_bounds_check_inner_kernel<d()>), dim3((unsigned)g), dim3(kBlock),
                               sizeof(uint4) * (size_t)(a.v.N + 1), st, a, k, i0, ni);
        });
        return hipGetLastError();
    }
    for_assets(a.d, [&](auto d) {
        hipLaunchKernelGGL((basket_bounds_check_inner_kernel<d()>), dim3((unsigned)g), dim3(kBlock),
                           sizeof(uint4) * (size_t)(a.v.N + 1), st, a, k, i0, ni);
    });
    return hipGetLastError();
}

}  // namespace omc
