// omc_bounds.hip -- Andersen-Broadie price bounds of the Bermudan option on the pricing grid.
//
// Three sweeps, all with one frozen exercise policy (betas [N+1][4]) and GBM paths from the generator's own Philox
// counters and spot recurrence:
//   lower   one thread per antithetic pair of fresh paths, in registers: each partner stops at the FIRST date the rule
//           fires (or N) and contributes Z = exp(-r tau dt) max(phi, 0); pair means reduced per workgroup.
//   inner   the hot path: for every (outer path i, date t) item the mean Q^_t[i] of Z at tau_{t+1} over n_inner inner
//           paths started at the outer spot S_t[i].  A wave owns one item at a time; each lane simulates one antithetic
//           inner PAIR four steps per Philox block and, when both partners have stopped, takes the item's next
//           unstarted pair -- inner paths end anywhere between 1 and N - t steps, and only the item's tail is lost to
//           lanes without work.
//   walk    one thread per outer pair: L^, M^ and max_t (Z_t - M^_t) per outer path, pair means reduced per workgroup.
// Decisions: pass 2's float32 exercise tables (omc_crit.h, the stored-path kind) -- two unsigned compares on the spot's
// bits -- and, on the steps the table builder marks irregular, the float64 rule itself.  Both give the same decisions.
// Sums: float64, per lane in a fixed order, per wave / workgroup in a fixed tree, then lsm_finalize: identical calls
// return identical bits (the inner step count is an integer atomic sum, exact in any order).
#include "omc_bounds_dev.h"

namespace omc {

// ------------------------------------------------------------------ lower bound
__global__ __launch_bounds__(kBlock) void bounds_lower_kernel(BoundsArgs a, int nblk)
{
    extern __shared__ uint4 sh_bt[];
    __shared__ double red[kNQ * kRedStride];
    bd_load_tables(a, sh_bt);
    const int N = a.N;
    double acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0;
    const int64_t P = a.n_lower / 2;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < P; p += (int64_t)nblk * kBlock) {
        float sa = a.s0, sb = a.s0, xa = a.s0, xb = a.s0;
        int da = 0, db = 0;  // stop dates, 0 while live
        for (int blk = 0; 4 * blk < N && (da == 0 || db == 0); ++blk) {
            float z[4];
            normals4((uint64_t)p, (uint32_t)blk, a.stream_lower, a.k0, a.k1, z);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int d = 4 * blk + u + 1;
                if (d > N) break;
                sa = sa * fast_exp2(__builtin_fmaf(a.b, z[u], a.a));
                sb = sb * fast_exp2(__builtin_fmaf(-a.b, z[u], a.a));
                const uint4 iv = sh_bt[d];
                const bool ea = da == 0 && bd_stop(sa, d, iv, a);
                const bool eb = db == 0 && bd_stop(sb, d, iv, a);
                xa = ea ? sa : xa;
                da = ea ? d : da;
                xb = eb ? sb : xb;
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

int64_t bounds_lower_blocks(const BoundsArgs& a)
{
    const int64_t P = a.n_lower / 2;
    const int64_t b = (P + kBlock - 1) / kBlock;
    return b < kMaxLsmBlocks ? b : kMaxLsmBlocks;
}

hipError_t bounds_lower(hipStream_t st, const BoundsArgs& a, double* result)
{
    const int nblk = (int)bounds_lower_blocks(a);
    hipLaunchKernelGGL(bounds_lower_kernel, dim3(nblk), dim3(kBlock), sizeof(uint4) * (size_t)(a.N + 1), st, a, nblk);
    return lsm_finalize(st, a.part, nullptr, result, nblk, 0);
}

// ------------------------------------------------------------------ inner simulations
// items q = t * ni + (i - i0): all outer paths of the earliest date first, so the longest items start first
__global__ __launch_bounds__(kBlock) void bounds_inner_kernel(BoundsArgs a, int64_t i0, int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bd_load_tables(a, sh_bt);
    const int N = a.N;
    const int lane = (int)(threadIdx.x & 63);
    const int64_t H = a.half_inner;
    const int64_t n_items = ni * N;
    const int64_t nwaves = (int64_t)gridDim.x * (kBlock / 64);
    unsigned long long steps = 0;
    for (int64_t item = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); item < n_items; item += nwaves) {
        const int t = (int)(item / ni);
        const int64_t i = i0 + (item - (int64_t)t * ni);
        const float s0 = a.So[(size_t)t * a.n_outer + i];
        const uint64_t gbase = ((uint64_t)i * (uint64_t)(N + 1) + (uint64_t)t) * (uint64_t)H;
        int64_t j = lane, next = 64;  // this lane's pair; the item's first unstarted pair
        bool act = j < H;
        float sa = s0, sb = s0, xa = s0, xb = s0;
        int k = 0, da = 0, db = 0;  // steps taken by the pair; stop dates of its partners (0 while live)
        double acc = 0.0;
        while (__builtin_amdgcn_ballot_w64(act)) {
            if (act) {
                float z[4];
                normals4(gbase + (uint64_t)j, (uint32_t)(k >> 2), a.stream_inner, a.k0, a.k1, z);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (da == 0 || db == 0) {
                        ++k;
                        const int d = t + k;
                        sa = sa * fast_exp2(__builtin_fmaf(a.b, z[u], a.a));
                        sb = sb * fast_exp2(__builtin_fmaf(-a.b, z[u], a.a));
                        const uint4 iv = sh_bt[d];
                        const bool ea = da == 0 && bd_stop(sa, d, iv, a);
                        const bool eb = db == 0 && bd_stop(sb, d, iv, a);
                        xa = ea ? sa : xa;
                        da = ea ? d : da;
                        xb = eb ? sb : xb;
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
                sa = sb = xa = xb = s0;
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

hipError_t bounds_inner(hipStream_t st, const BoundsArgs& a, int64_t i0, int64_t ni)
{
    const int64_t items = ni * a.N;
    int64_t g = (items + 3) / 4;
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(bounds_inner_kernel, dim3((unsigned)g), dim3(kBlock), sizeof(uint4) * (size_t)(a.N + 1), st, a,
                       i0, ni);
    return hipGetLastError();
}

// ------------------------------------------------------------------ outer walk
__device__ __forceinline__ double bd_sample(const BoundsArgs& a, int64_t i)
{
    const int N = a.N;
    const double* q = a.q + (size_t)i * N;
    double M = 0.0, qprev = q[0], best = -__builtin_huge_val();
    for (int t = 1; t <= N; ++t) {
        const float s = a.So[(size_t)t * a.n_outer + i];
        const double Z = bd_value(s, t, a);
        const uint4 iv = *reinterpret_cast<const uint4*>(a.tab + (size_t)t * 8);
        const double qt = t < N ? q[t] : 0.0;
        const double L = bd_stop(s, t, iv, a) ? Z : qt;
        M = M + L - qprev;
        const double x = Z - M;
        best = x > best ? x : best;
        qprev = qt;
    }
    return best;
}

__global__ __launch_bounds__(kBlock) void bounds_walk_kernel(BoundsArgs a, int nblk)
{
    __shared__ double red[kNQ * kRedStride];
    double acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0;
    const int64_t P = a.n_outer / 2;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < P; p += (int64_t)nblk * kBlock) {
        const double xa = bd_sample(a, p), xb = bd_sample(a, p + P);
        a.samples[p] = xa;
        a.samples[p + P] = xb;
        const double m = 0.5 * (xa + xb);
        acc[0] += m;
        acc[1] += m * m;
    }
    const double s = block_reduce8(acc, red);
    if (threadIdx.x < 64 && (threadIdx.x & 7) == 0) a.part[(size_t)(threadIdx.x >> 3) * kPStride + blockIdx.x] = s;
}

int64_t bounds_walk_blocks(const BoundsArgs& a)
{
    const int64_t b = (a.n_outer / 2 + kBlock - 1) / kBlock;
    return b < kMaxLsmBlocks ? b : kMaxLsmBlocks;
}

hipError_t bounds_walk(hipStream_t st, const BoundsArgs& a, double* result)
{
    const int nblk = (int)bounds_walk_blocks(a);
    hipLaunchKernelGGL(bounds_walk_kernel, dim3(nblk), dim3(kBlock), 0, st, a, nblk);
    return lsm_finalize(st, a.part, nullptr, result, nblk, 0);
}

}  // namespace omc
