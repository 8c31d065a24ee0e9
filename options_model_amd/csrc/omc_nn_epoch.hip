// omc_nn_epoch.hip -- what an epoch of the NN regressor needs around the network arithmetic.  In this file:
//   * nn_stats_kernel / nn_stats_finish_kernel / nn_feature_stats: float64 means and variances of the regression
//     features and the target (the normalisers);
//   * mlp_shuffle_kernel / mlp_shuffle_indices: the keyed permutation an epoch walks, written out (for tests);
//   * shard_select / shard_gather / shard_step_off kernels behind mlp_shard_select and mlp_shard_gather: this rank's
//     rows of a sharded epoch's global minibatches.
// The permutation itself (Shuffle, shuffle_index, make_shuffle) is in omc_mlp_dev.h: the trainers evaluate it too.
#include "omc_mlp_dev.h"

namespace omc {

namespace {

// ------------------------------------------------------------------ feature statistics
// Means and population variances of the six non-constant regression features
// [x, x^2, x^3, max(x-1,0), s, x*s] (create_regression_features, options_model_3.py:105-121;
// s = sqrt(max(T - t*dt, 1e-6))) and of the target over all R rows, in float64
// (:550-563).  PASS 0 sums values, PASS 1 sums squared deviations from the given means.
struct StatArgs {
    const double* x;
    const int32_t* t;
    const double* y;
    int64_t n;
    double T, dt;
    const double* mean;  // [8] (PASS 1)
    double* part;        // [8][pstride]
    int pstride;
};

template <int PASS>
__global__ __launch_bounds__(kBlock) void nn_stats_kernel(StatArgs a)
{
    __shared__ double red[kNQ * kRedStride];
    double acc[8], mu[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        acc[q] = 0.0;
        mu[q] = PASS ? a.mean[q] : 0.0;
    }
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += stride) {
        const double x = a.x[i];
        const double s = sqrt(fmax(a.T - (double)a.t[i] * a.dt, 1e-6));
        const double x2 = x * x;
        const double f[8] = {x, x2, x2 * x, fmax(x - 1.0, 0.0), s, x * s, a.y[i], 0.0};
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            const double d = f[q] - mu[q];
            acc[q] += PASS ? d * d : d;
        }
    }
    const double r = block_reduce8(acc, red);
    if (threadIdx.x < 64 && (threadIdx.x & 7) == 0)
        a.part[(size_t)(threadIdx.x >> 3) * a.pstride + blockIdx.x] = r;
}

// part[q][0..nblk) summed in index order, divided by n -> out[q]
__global__ __launch_bounds__(kBlock) void nn_stats_finish_kernel(const double* part, int nblk, int pstride,
                                                                double n, double* out)
{
    __shared__ double red[kNQ * kRedStride];
    double acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0;
    for (int i = threadIdx.x; i < nblk; i += kBlock) {
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] += part[(size_t)q * pstride + i];
    }
    const double r = block_reduce8(acc, red);
    if (threadIdx.x < 64 && (threadIdx.x & 7) == 0) out[threadIdx.x >> 3] = r / n;
}

// ------------------------------------------------------------------ epoch order, sharded epochs
__global__ __launch_bounds__(256) void mlp_shuffle_kernel(Shuffle s, int64_t* out)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < s.n) out[i] = (int64_t)shuffle_index(s, i);
}

// ---- sharded epochs: this rank's positions of the epoch's keyed permutation over ALL ranks' rows
struct ShardSel {
    Shuffle sh;             // permutation of [0, rows_global)
    const int64_t* gstart;  // [nseg + 1]
    const int64_t* lstart;  // [nseg], -1 = not this rank's
    int nseg;
    int group;              // segments per time step (2 x ranks): the table is searched in two levels -- the step in LDS
                            // (nseg / group + 1 starts), the segment inside the step's `group` entries; 0: flat search
};
constexpr int kSelPerThread = 16, kSelPerBlock = 256 * kSelPerThread;
constexpr int kSelMaxSteps = 4096;  // step starts staged in LDS (32 KB); longer tables are searched flat

// own row of global row g, or -1: the LAST segment that starts at or before g (empty segments share a start)
__device__ __forceinline__ int64_t shard_locate(const ShardSel& s, const int64_t* __restrict__ step_start, int nsteps,
                                                int64_t g)
{
    int lo = 0, hi = s.nseg;  // gstart[lo] <= g < gstart[hi]
    if (step_start) {
        int a = 0, b = nsteps;  // step_start[a] <= g < step_start[b]
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (step_start[mid] <= g) a = mid;
            else b = mid;
        }
        lo = a * s.group;
        hi = min(lo + s.group, s.nseg);
    }
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (s.gstart[mid] <= g) lo = mid;
        else hi = mid;
    }
    const int64_t l = s.lstart[lo];
    return l < 0 ? -1 : l + (g - s.gstart[lo]);
}

// Every rank walks ALL epoch positions (ownership is only known after the permutation is evaluated), so this is the one
// per-rank cost of a sharded epoch that does not shrink with the number of ranks: 16 positions per thread, the
// time-step starts of the segment table in LDS.  WRITE = false: which of a thread's 16 positions are this rank's ->
// mask[thread] (a bit each), cnt[block] = their number.  WRITE = true: only the positions with a bit set are evaluated
// again (1 / ranks of them) and written, ascending, at offs[block] + rank inside the block.
template <bool WRITE>
__global__ __launch_bounds__(256) void shard_select_kernel(ShardSel s, int32_t* __restrict__ cnt, uint16_t* __restrict__ mask,
                                                           const int64_t* __restrict__ offs, int64_t* __restrict__ sel_row,
                                                           int64_t* __restrict__ sel_i)
{
    __shared__ int scan[256];
    __shared__ int64_t sh_step[kSelMaxSteps + 1];
    const int tid = threadIdx.x;
    const int nsteps = s.group > 0 ? s.nseg / s.group : 0;
    const int64_t* step_start = nullptr;
    if (nsteps > 0 && nsteps <= kSelMaxSteps && nsteps * s.group == s.nseg) {
        for (int i = tid; i <= nsteps; i += 256) sh_step[i] = s.gstart[min(i * s.group, s.nseg)];
        __syncthreads();
        step_start = sh_step;
    }
    const uint64_t i0 = (uint64_t)blockIdx.x * kSelPerBlock + (uint64_t)tid * kSelPerThread;
    const size_t slot = (size_t)blockIdx.x * 256 + tid;
    if (!WRITE) {
        unsigned m = 0;
#pragma unroll 4
        for (int j = 0; j < kSelPerThread; ++j) {
            const uint64_t i = i0 + j;
            if (i < s.sh.n && shard_locate(s, step_start, nsteps, (int64_t)shuffle_index(s.sh, i)) >= 0) m |= 1u << j;
        }
        mask[slot] = (uint16_t)m;
        int n = __builtin_popcount(m);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) n += __shfl_down(n, d, 64);
        if ((tid & 63) == 0) scan[tid >> 6] = n;
        __syncthreads();
        if (tid == 0) cnt[blockIdx.x] = scan[0] + scan[1] + scan[2] + scan[3];
        return;
    }
    const unsigned m = mask[slot];
    const int n = __builtin_popcount(m);
    scan[tid] = n;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {  // inclusive scan of the threads' counts
        const int v = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    int64_t o = offs[blockIdx.x] + (scan[tid] - n);
    for (unsigned r = m; r; r &= r - 1) {
        const int j = __builtin_ctz(r);
        const uint64_t i = i0 + j;
        sel_row[o] = shard_locate(s, step_start, nsteps, (int64_t)shuffle_index(s.sh, i));
        sel_i[o] = (int64_t)i;
        ++o;
    }
}

__global__ __launch_bounds__(256) void shard_gather_kernel(const float4* __restrict__ data, const int64_t* __restrict__ sel_row,
                                                           const int64_t* __restrict__ sel_i, int64_t n, int64_t batch,
                                                           float4* __restrict__ out, uint32_t* __restrict__ drop_pos)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;  // one thread per half row (16 bytes)
    const int64_t j = t >> 1;
    if (j >= n) return;
    const int h = (int)(t & 1);
    out[j * 2 + h] = data[sel_row[j] * 2 + h];
    if (h == 0) drop_pos[j] = (uint32_t)(sel_i[j] % batch);
}

// step_off[k] = first j with sel_i[j] >= k * batch (sel_i ascending), k = 0 .. steps
__global__ __launch_bounds__(256) void shard_step_off_kernel(const int64_t* __restrict__ sel_i, int64_t n, int64_t batch,
                                                             int64_t steps, int64_t* __restrict__ step_off)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > steps) return;
    const int64_t key = k * batch;
    int64_t lo = 0, hi = n;  // first index with sel_i >= key
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (sel_i[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    step_off[k] = lo;
}

}  // namespace

size_t nn_stats_scratch_bytes() { return sizeof(double) * 8 * (1024 + 2); }

// out[0..7] = means, out[8..15] = population variances (slots 0-5 features 1..6, slot 6 target)
hipError_t nn_feature_stats(hipStream_t st, const double* x, const int32_t* t, const double* y, int64_t n,
                            double T, double dt, double* scratch, double* out16)
{
    StatArgs a;
    a.x = x; a.t = t; a.y = y; a.n = n; a.T = T; a.dt = dt;
    a.part = scratch; a.pstride = 1024; a.mean = out16;
    int nblk = (int)((n + kBlock * 8 - 1) / (kBlock * 8));
    nblk = nblk < 1 ? 1 : (nblk > 1024 ? 1024 : nblk);
    hipLaunchKernelGGL(nn_stats_kernel<0>, dim3(nblk), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(nn_stats_finish_kernel, dim3(1), dim3(kBlock), 0, st, scratch, nblk, 1024, (double)n, out16);
    hipLaunchKernelGGL(nn_stats_kernel<1>, dim3(nblk), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(nn_stats_finish_kernel, dim3(1), dim3(kBlock), 0, st, scratch, nblk, 1024, (double)n, out16 + 8);
    return hipGetLastError();
}

hipError_t mlp_shuffle_indices(hipStream_t st, int64_t n, uint64_t shuffle_key, int64_t* out)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(mlp_shuffle_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                       make_shuffle(n, shuffle_key), out);
    return hipGetLastError();
}

size_t mlp_shard_scratch_bytes(int64_t rows_global)
{
    const size_t nb = (size_t)((rows_global + kSelPerBlock - 1) / kSelPerBlock);
    return sizeof(int64_t) * (nb + 2) + sizeof(int32_t) * (nb + 2) + sizeof(uint16_t) * 256 * (nb + 1) + 64;
}

hipError_t mlp_shard_select(hipStream_t st, int64_t rows_global, uint64_t shuffle_key, const int64_t* gstart,
                            const int64_t* lstart, int nseg, int group, void* scratch, int64_t* sel_row, int64_t* sel_i,
                            const int64_t** total_dev)
{
    const int64_t nb = (rows_global + kSelPerBlock - 1) / kSelPerBlock;
    int64_t* offs = (int64_t*)scratch;
    int32_t* cnt = (int32_t*)(offs + nb + 2);
    uint16_t* mask = (uint16_t*)(((uintptr_t)(cnt + nb + 2) + 15) & ~(uintptr_t)15);
    *total_dev = offs + nb;
    if (nb == 0 || nseg <= 0) return hipMemsetAsync(offs, 0, sizeof(int64_t) * (size_t)(nb + 1), st);
    ShardSel s;
    s.sh = make_shuffle(rows_global, shuffle_key);
    s.gstart = gstart; s.lstart = lstart; s.nseg = nseg; s.group = group;
    hipLaunchKernelGGL(shard_select_kernel<false>, dim3((unsigned)nb), dim3(256), 0, st, s, cnt, mask, (const int64_t*)nullptr,
                       (int64_t*)nullptr, (int64_t*)nullptr);
    hipError_t e = nn_scan_counts(st, cnt, nb, offs);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(shard_select_kernel<true>, dim3((unsigned)nb), dim3(256), 0, st, s, cnt, mask, (const int64_t*)offs,
                       sel_row, sel_i);
    return hipGetLastError();
}

hipError_t mlp_shard_gather(hipStream_t st, const float* data, const int64_t* sel_row, const int64_t* sel_i,
                            int64_t n_local, int64_t batch, int64_t steps, float* data_epoch, uint32_t* drop_pos,
                            int64_t* step_off)
{
    if (n_local > 0)
        hipLaunchKernelGGL(shard_gather_kernel, dim3((unsigned)((2 * n_local + 255) / 256)), dim3(256), 0, st,
                           (const float4*)data, sel_row, sel_i, n_local, batch, (float4*)data_epoch, drop_pos);
    hipLaunchKernelGGL(shard_step_off_kernel, dim3((unsigned)((steps + 1 + 255) / 256)), dim3(256), 0, st, sel_i, n_local, batch,
                       steps, step_off);
    return hipGetLastError();
}

}  // namespace omc
