// omc_mlp_batch.hip -- many small networks of one shape trained side by side (the curve entry points: one net per
// curve point; the per-step ContNet flow of a curve: one net per point and time step).  In this file:
//   * MlpBatchProb, the device table with one row per network, and its host image (mlp_batch_table_image);
//   * mlp_train_quad_batch_kernel (blockIdx.y = network) and mlp_train_quad_list_kernel (a work list of (network,
//     tile) items for batches of very uneven sizes, with mlp_tile_prefix_kernel) around the tile-per-workgroup
//     bodies of omc_mlp_quad_dev.h, mlp_adam_batch_kernel, mlp_transpose_batch_kernel;
//   * their launchers: mlp_train_epoch_batch, mlp_train_step_batch, mlp_tile_prefix.
// A workgroup gets its network's argument blocks from mlp_step_args / mlp_adam_args (omc_mlp_dev.h), the functions
// the host loop of omc_mlp.hip calls, and runs the single-network body: every network ends an epoch with the bits of
// its own omc_mlp_train_epoch call (tests/test_gpu_nn_curve.py, test_gpu_contnet_batch.py).
#include "omc_mlp_quad_dev.h"

#include <cstring>

namespace omc {

namespace {

// One table row per problem; the step index within the epoch is a kernel argument.  Problems whose epoch is shorter
// leave at once.
struct MlpBatchProb {
    MlpNet net;
    int64_t nrows, batch, first_step;
    int q16_rows;  // minibatches of up to so many rows run in 16-row tiles (0: never)
    // non-null: the set size lives in device memory (the per-step ContNet flow: the regression set of the step,
    // counted by the kernels right before): nrows = batch = (int64_t)*nrows_dev, read when the kernel runs
    const double* nrows_dev;
};

__device__ __forceinline__ void batch_rows(const MlpBatchProb& p, int64_t* nrows, int64_t* batch)
{
    if (p.nrows_dev) {
        *nrows = *batch = (int64_t)*p.nrows_dev;
    } else {
        *nrows = p.nrows;
        *batch = p.batch;
    }
}

// Q16: this launch serves the problems whose minibatch runs in 16-row tiles (the kernel their single call runs,
// mlp_train_kernel_choice); the others leave at once -- and the other way round in the 32-row launch.
template <int H, int L, bool Q16 = false>
__global__ __launch_bounds__(H * 2) void mlp_train_quad_batch_kernel(const MlpBatchProb* __restrict__ tab, int s,
                                                                     int step_base)
{
    const MlpBatchProb& p = tab[blockIdx.y];
    const int tile = blockIdx.x;
    int64_t nrows, batch;
    batch_rows(p, &nrows, &batch);
    if ((batch <= (int64_t)p.q16_rows) != Q16) return;
    const int64_t o = (int64_t)s * batch;
    if (o >= nrows) return;
    const int64_t nb = (nrows - o < batch) ? nrows - o : batch;
    const MlpStepArgs a = mlp_step_args(p.net, o, nb, nb, Q16 ? 16 : 32, p.first_step + step_base + s + 1);
    if constexpr (Q16) mlp_train_q16_body<H, L>(a, tile);  // (the grid covers the largest problem's tiles)
    else mlp_train_quad_body<H, L>(a, tile);
}

// Work-list form of the same launch for batches whose problems differ wildly in size (the per-step ContNet flow of
// a curve: at any loop step a few problems are at their first regression step with thousands of rows while the rest
// have a few dozen): `prefix[p]` = tiles of problems 0 .. p-1 (mlp_tile_prefix_kernel, once per time step), the
// grid's workgroups share the total evenly, each walking a contiguous run of (problem, tile) items.  One partial per
// tile as before, so nothing changes for the sums.
__global__ __launch_bounds__(1024) void mlp_tile_prefix_kernel(const MlpBatchProb* __restrict__ tab, int n,
                                                              int* __restrict__ prefix)
{
    __shared__ int seg[1024];
    const int tid = threadIdx.x;
    const int len = (n + 1023) / 1024, lo = tid * len, hi = lo + len < n ? lo + len : n;
    int s = 0;
    for (int i = lo; i < hi; ++i) {
        int64_t nrows, batch;
        batch_rows(tab[i], &nrows, &batch);
        const int64_t nb = nrows < batch ? nrows : batch;
        s += (int)((nb + 31) / 32);
    }
    seg[tid] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = tid >= d ? seg[tid - d] : 0;
        __syncthreads();
        seg[tid] += v;
        __syncthreads();
    }
    int run = tid ? seg[tid - 1] : 0;
    for (int i = lo; i < hi; ++i) {
        prefix[i] = run;
        int64_t nrows, batch;
        batch_rows(tab[i], &nrows, &batch);
        const int64_t nb = nrows < batch ? nrows : batch;
        run += (int)((nb + 31) / 32);
    }
    if (tid == 1023) prefix[n] = seg[1023];
}

template <int H, int L>
__global__ __launch_bounds__(H * 2) void mlp_train_quad_list_kernel(const MlpBatchProb* __restrict__ tab,
                                                                    const int* __restrict__ prefix, int n, int step_base)
{
    const int total = prefix[n];
    const int per = (total + (int)gridDim.x - 1) / (int)gridDim.x;
    int item = (int)blockIdx.x * per;
    const int end = item + per < total ? item + per : total;
    if (item >= end) return;
    int lo = 0, hi = n;  // the problem that owns `item`: the last p with prefix[p] <= item
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= item) lo = mid; else hi = mid;
    }
    int p = lo;
    while (item < end) {
        while (prefix[p + 1] <= item) ++p;  // (problems without tiles are skipped)
        const MlpBatchProb& pb = tab[p];
        int64_t nrows, batch;
        batch_rows(pb, &nrows, &batch);
        const int64_t nb = nrows < batch ? nrows : batch;
        const MlpStepArgs a = mlp_step_args(pb.net, 0, nb, nb, 32, pb.first_step + step_base + 1);
        const int first = prefix[p];
        const int last = prefix[p + 1] < end ? prefix[p + 1] : end;
        for (; item < last; ++item) {
            mlp_train_quad_body<H, L>(a, item - first);
            __syncthreads();
        }
    }
}

// bc1 / bc2: 1 - beta^step for step = 0 .. (host-computed tables: libm pow, as the host loop uses)
template <bool FLAT>
__global__ __launch_bounds__(256) void mlp_adam_batch_kernel(const MlpBatchProb* __restrict__ tab, int s, int step_base,
                                                            int H, int L, const double* __restrict__ bc1,
                                                            const double* __restrict__ bc2)
{
    const MlpBatchProb& p = tab[blockIdx.y];
    int64_t nrows, batch;
    batch_rows(p, &nrows, &batch);
    const int64_t o = (int64_t)s * batch;
    if (o >= nrows) return;
    const int64_t nb = (nrows - o < batch) ? nrows - o : batch;
    const int64_t step = p.first_step + step_base + s + 1;
    const int nparts = batch <= (int64_t)p.q16_rows ? (int)((nb + 15) / 16) : (int)((nb + 31) / 32);  // one partial per tile
    const MlpAdamArgs b = mlp_adam_args(p.net, nparts, H, L, nb, bc1[step], bc2[step]);
    // FLAT: one thread per parameter (few, full workgroups: many problems per launch); else 16 threads per parameter
    // (the single-problem kernel's shape: shortest latency for a lone problem).  Same bits either way.
    if constexpr (FLAT) mlp_adam_body_flat(b, (int)(blockIdx.x * 256 + threadIdx.x));
    else mlp_adam_body(b);
}

// wt_j[k][i] = W_j[i][k] for the L-1 connections of every problem (start of an epoch; Adam keeps it current)
__global__ __launch_bounds__(256) void mlp_transpose_batch_kernel(const MlpBatchProb* __restrict__ tab, int H, int L)
{
    const MlpNet& p = tab[blockIdx.y].net;
    const int n = (L - 1) * H * H;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int j = i / (H * H), rem = i - j * H * H, k = rem / H, u = rem - k * H;
        p.wt[i] = p.params[H * 8 + (size_t)j * (H * H + H) + (size_t)u * H + k];
    }
}

}  // namespace

size_t mlp_batch_table_bytes(int n) { return sizeof(MlpBatchProb) * (size_t)n; }

void mlp_batch_table_image(const MlpBatchJob* jobs, int n, int hidden, int layers, double beta1, double beta2, double eps,
                           double weight_decay, double dropout, void* out)
{
    MlpBatchProb* tab = (MlpBatchProb*)out;
    for (int i = 0; i < n; ++i) {
        const MlpBatchJob& j = jobs[i];
        MlpBatchProb& p = tab[i];
        memset(&p, 0, sizeof p);
        p.net = mlp_net(j.data, j.params, j.adam_m, j.adam_v, j.partial, j.wt, j.loss_acc, j.lr, beta1, beta2, eps,
                        weight_decay, make_shuffle(j.nrows, j.shuffle_key), dropout, j.seed, tile_pstride(hidden, layers));
        p.nrows = j.nrows; p.batch = j.batch; p.first_step = j.first_step;
        p.q16_rows = j.allow_q16 ? (int)mlp_q16_rows(hidden) : 0;
        p.nrows_dev = j.nrows_dev;
    }
}

// the Adam launch of a batch of n problems: one thread per parameter from 8 problems on
template <int H, int L>
static void launch_adam_batch(hipStream_t st, const MlpBatchProb* tab, int n, int s, int step_base, const double* bc1,
                              const double* bc2)
{
    constexpr int NP = mlp_params_of(H, L);
    if (n >= 8) hipLaunchKernelGGL(mlp_adam_batch_kernel<true>, dim3((NP + 256) / 256, (unsigned)n), dim3(256), 0, st, tab, s, step_base, H, L, bc1, bc2);
    else hipLaunchKernelGGL(mlp_adam_batch_kernel<false>, dim3((NP + 16) / 16, (unsigned)n), dim3(256), 0, st, tab, s, step_base, H, L, bc1, bc2);
}

// one epoch: one launch pair per optimizer step for ALL problems (hidden 32 / 64 / 128, 2 / 3 layers)
// max_tiles32 / max_tiles16: the largest minibatch among the problems that run in 32-row / in 16-row tiles (0: none)
hipError_t mlp_train_epoch_batch(hipStream_t st, const void* table_dev, int n, int hidden, int layers, int64_t max_steps,
                                 int max_tiles32, int max_tiles16, const double* bc1_dev, const double* bc2_dev)
{
    const MlpBatchProb* tab = (const MlpBatchProb*)table_dev;
    return dispatch_hl(hidden, layers, [&](auto h, auto l) -> hipError_t {
        constexpr int H = decltype(h)::value, L = decltype(l)::value;
        hipLaunchKernelGGL(mlp_transpose_batch_kernel, dim3(16, n), dim3(256), 0, st, tab, H, L);
        for (int64_t s = 0; s < max_steps; ++s) {
            // every problem runs the kernel its own omc_mlp_train_epoch call runs: one launch for the problems in 32-row
            // tiles, one for those in 16-row tiles (a curve's points normally all share the reference's minibatch of 256)
            if (max_tiles32 > 0)
                hipLaunchKernelGGL((mlp_train_quad_batch_kernel<H, L, false>), dim3((unsigned)max_tiles32, (unsigned)n), dim3(H * 2), 0,
                                   st, tab, (int)s, 0);
            if constexpr (H >= 64) {  // (32 units: no 16-row kernel)
                if (max_tiles16 > 0)
                    hipLaunchKernelGGL((mlp_train_quad_batch_kernel<H, L, true>), dim3((unsigned)max_tiles16, (unsigned)n), dim3(H * 2),
                                       0, st, tab, (int)s, 0);
            }
            launch_adam_batch<H, L>(st, tab, n, (int)s, 0, bc1_dev, bc2_dev);
        }
        return hipGetLastError();
    });
}

// ONE full-batch optimizer step (forward / backward + Adam) for every problem of the table: the per-step ContNet
// flow's "epoch" (hidden 32 / 64 / 128, two hidden layers).  `step_base` = optimizer steps the nets have taken so far
// (Adam's bias correction); the transposed connection copies must be current (the flow's init kernel writes them, Adam
// keeps them so).
hipError_t mlp_train_step_batch(hipStream_t st, const void* table_dev, int n, int hidden, int grid_tiles, int step_base,
                                const double* bc1_dev, const double* bc2_dev, const int* tile_prefix_dev)
{
    const MlpBatchProb* tab = (const MlpBatchProb*)table_dev;
    return dispatch_h(hidden, [&](auto h) -> hipError_t {
        constexpr int H = decltype(h)::value, L = 2;
        if (tile_prefix_dev)
            hipLaunchKernelGGL((mlp_train_quad_list_kernel<H, L>), dim3((unsigned)grid_tiles), dim3(H * 2), 0, st, tab, tile_prefix_dev, n, step_base);
        else
            hipLaunchKernelGGL((mlp_train_quad_batch_kernel<H, L, false>), dim3((unsigned)grid_tiles, (unsigned)n), dim3(H * 2), 0, st, tab, 0, step_base);
        launch_adam_batch<H, L>(st, tab, n, 0, step_base, bc1_dev, bc2_dev);
        return hipGetLastError();
    });
}

hipError_t mlp_tile_prefix(hipStream_t st, const void* table_dev, int n, int* prefix_dev)
{
    hipLaunchKernelGGL(mlp_tile_prefix_kernel, dim3(1), dim3(1024), 0, st, (const MlpBatchProb*)table_dev, n, prefix_dev);
    return hipGetLastError();
}

}  // namespace omc
