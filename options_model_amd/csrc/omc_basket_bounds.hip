// omc_basket_bounds.hip -- Andersen-Broadie price bounds on the index of D correlated GBM assets.
//
// The two sweeps of omc_bounds.hip that simulate paths, with D assets per partner:
//   lower   bounds_lower_kernel's shape: one thread per antithetic pair of fresh paths, both partners' D spots in
//           registers, each partner stopped at the first date the rule fires on its INDEX.
//   inner   bounds_inner_kernel's shape, the hot path: a wave per (outer path, date) item, a lane per antithetic inner
//           pair, four steps per Philox block per asset, finished lanes refilled from the item's unstarted pairs (ballot +
//           mbcnt), a fixed xor-shuffle sum, an integer atomic step count.  The item's D start spots are the outer ASSET
//           spots A_k[t][i]: loaded once per item, wave-uniform, kept in scalar registers.
// Every spot is the basket generator's (omc_basket.hip, include/omc.h): asset k of pair g draws normals4(g + (k << 40)),
// the correlated normals accumulate with k ascending in the generator's fmaf chain, the step is s *= exp2(fmaf(+-b_k, y_k,
// a_k)), the index is the generator's rule for the kind.  These three are restated here, not shared, so the generator's
// instruction streams stay what they were.  The law and the kind come by value; D is a template parameter so that every
// loop over assets unrolls and no array is indexed at run time (no scratch: section 17.3).
// With D = 1 and w = 1 both kernels perform the vanilla kernels' operations in the vanilla order: the same bits.
// The outer walk, the exercise tables and the finalize are omc_bounds.hip's / omc_lsm.hip's, on the index matrix.
#include "omc_basket_bounds.h"
#include "omc_bounds_dev.h"

#include "../../include/omc.h"

namespace omc {

// the correlated normals of one pair's Philox block `blk`: y[i][j] for asset i, step j of the block
template <int D>
__device__ __forceinline__ void bb_normals(const BasketLaw& c, uint64_t pair, uint32_t blk, uint32_t stream, uint32_t k0,
                                           uint32_t k1, float (&y)[D][4])
{
#pragma unroll
    for (int k = 0; k < D; ++k) {
        float z[4];
        normals4(pair + ((uint64_t)k << 40), blk, stream, k0, k1, z);
#pragma unroll
        for (int i = k; i < D; ++i) {
            const float l = c.L[i * (i + 1) / 2 + k];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i == 0) y[i][j] = z[j];  // Lf[0][0] = 1.0f exactly
                else if (k == 0) y[i][j] = l * z[j];
                else y[i][j] = __builtin_fmaf(l, z[j], y[i][j]);
            }
        }
    }
}

template <int KIND, int D>
__device__ __forceinline__ float bb_index_of(const BasketLaw& c, const float (&s)[D])
{
    float x = c.w[0] * s[0];
#pragma unroll
    for (int k = 1; k < D; ++k) {
        if constexpr (KIND == OMC_BASKET_ARITHMETIC) x = __builtin_fmaf(c.w[k], s[k], x);
        else if constexpr (KIND == OMC_BASKET_BEST_OF) x = fmaxf(x, c.w[k] * s[k]);
        else x = fminf(x, c.w[k] * s[k]);
    }
    return x;
}

// (the kind is wave-uniform: a scalar branch)
template <int D>
__device__ __forceinline__ float bb_index(const BasketLaw& c, const float (&s)[D])
{
    if (c.kind == OMC_BASKET_ARITHMETIC) return bb_index_of<OMC_BASKET_ARITHMETIC, D>(c, s);
    if (c.kind == OMC_BASKET_BEST_OF) return bb_index_of<OMC_BASKET_BEST_OF, D>(c, s);
    return bb_index_of<OMC_BASKET_WORST_OF, D>(c, s);
}

// one step of both partners' assets with the block's normals of step u
template <int D>
__device__ __forceinline__ void bb_step(const BasketLaw& c, float (&sa)[D], float (&sb)[D], const float (&y)[D][4], int u)
{
#pragma unroll
    for (int k = 0; k < D; ++k) {
        sa[k] = sa[k] * fast_exp2(__builtin_fmaf(c.b[k], y[k][u], c.a[k]));
        sb[k] = sb[k] * fast_exp2(__builtin_fmaf(-c.b[k], y[k][u], c.a[k]));
    }
}

// ------------------------------------------------------------------ lower bound
template <int D>
__global__ __launch_bounds__(kBlock) void basket_bounds_lower_kernel(BasketBoundsArgs g, int nblk)
{
    extern __shared__ uint4 sh_bt[];
    __shared__ double red[kNQ * kRedStride];
    const BoundsArgs& a = g.v;
    const BasketLaw& c = g.law;
    bd_load_tables(a, sh_bt);
    const int N = a.N;
    double acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0;
    const int64_t P = a.n_lower / 2;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < P; p += (int64_t)nblk * kBlock) {
        float sa[D], sb[D], xa = 0.0f, xb = 0.0f;  // the partners' asset spots; the index each stopped at
#pragma unroll
        for (int k = 0; k < D; ++k) sa[k] = sb[k] = c.s0[k];
        int da = 0, db = 0;  // stop dates, 0 while live
        for (int blk = 0; 4 * blk < N && (da == 0 || db == 0); ++blk) {
            float y[D][4];
            bb_normals<D>(c, (uint64_t)p, (uint32_t)blk, a.stream_lower, a.k0, a.k1, y);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int d = 4 * blk + u + 1;
                if (d > N) break;
                bb_step<D>(c, sa, sb, y, u);
                const float ia = bb_index<D>(c, sa), ib = bb_index<D>(c, sb);
                const uint4 iv = sh_bt[d];
                const bool ea = da == 0 && bd_stop(ia, d, iv, a);
                const bool eb = db == 0 && bd_stop(ib, d, iv, a);
                xa = ea ? ia : xa;
                da = ea ? d : da;
                xb = eb ? ib : xb;
                db = eb ? d : db;
            }
        }
        const double m = 0.5 * (bd_value(xa, da, a) + bd_value(xb, db, a));
        acc[0] += m;
        acc[1] += m * m;
        acc[2] += (da < N ? 1.0 : 0.0) + (db < N ? 1.0 : 0.0);
    }
    const double s = block_reduce8(acc, red);
    if (threadIdx.x < 64 && (threadIdx.x & 7) == 0) a.part[(size_t)(threadIdx.x >> 3) * kPStride + blockIdx.x] = s;
}

// ------------------------------------------------------------------ inner simulations
// items q = t * ni + (i - i0): all outer paths of the earliest date first, so the longest items start first
template <int D>
__global__ __launch_bounds__(kBlock) void basket_bounds_inner_kernel(BasketBoundsArgs g, int64_t i0, int64_t ni)
{
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
                bb_normals<D>(c, gbase + (uint64_t)j, (uint32_t)(k >> 2), a.stream_inner, a.k0, a.k1, y);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (da == 0 || db == 0) {
                        ++k;
                        const int d = t + k;
                        bb_step<D>(c, sa, sb, y, u);
                        const float ia = bb_index<D>(c, sa), ib = bb_index<D>(c, sb);
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

// ------------------------------------------------------------------ launchers
template <int D>
static void launch_lower(hipStream_t st, const BasketBoundsArgs& a, int nblk)
{
    hipLaunchKernelGGL((basket_bounds_lower_kernel<D>), dim3(nblk), dim3(kBlock), sizeof(uint4) * (size_t)(a.v.N + 1), st, a,
                       nblk);
}

template <int D>
static void launch_inner(hipStream_t st, const BasketBoundsArgs& a, unsigned grid, int64_t i0, int64_t ni)
{
    hipLaunchKernelGGL((basket_bounds_inner_kernel<D>), dim3(grid), dim3(kBlock), sizeof(uint4) * (size_t)(a.v.N + 1), st, a,
                       i0, ni);
}

#define OMC_BASKET_D_SWITCH(d, call)  \
    switch (d) {                      \
    case 1: call(1); break;           \
    case 2: call(2); break;           \
    case 3: call(3); break;           \
    case 4: call(4); break;           \
    case 5: call(5); break;           \
    case 6: call(6); break;           \
    case 7: call(7); break;           \
    default: call(8); break;          \
    }

hipError_t basket_bounds_lower(hipStream_t st, const BasketBoundsArgs& a, double* result)
{
    if (a.d < 1 || a.d > kBasketMax) return hipErrorInvalidValue;
    const int nblk = (int)bounds_lower_blocks(a.v);  // the vanilla sweep's grid
#define OMC_CALL(D) launch_lower<D>(st, a, nblk)
    OMC_BASKET_D_SWITCH(a.d, OMC_CALL)
#undef OMC_CALL
    return lsm_finalize(st, a.v.part, nullptr, result, nblk, 0);
}

hipError_t basket_bounds_inner(hipStream_t st, const BasketBoundsArgs& a, int64_t i0, int64_t ni)
{
    if (a.d < 1 || a.d > kBasketMax) return hipErrorInvalidValue;
    const int64_t items = ni * a.v.N;
    int64_t g = (items + 3) / 4;
    if (g > 2048) g = 2048;
#define OMC_CALL(D) launch_inner<D>(st, a, (unsigned)g, i0, ni)
    OMC_BASKET_D_SWITCH(a.d, OMC_CALL)
#undef OMC_CALL
    return hipGetLastError();
}

}  // namespace omc
