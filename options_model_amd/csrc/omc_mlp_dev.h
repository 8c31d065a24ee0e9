// omc_mlp_dev.h -- what the network kernels share on the device, and the one description of an optimizer step that
// the host loop and the side-by-side kernels both fill in.  Included by omc_mlp.hip (trainers), omc_mlp_batch.hip
// (many nets per launch), omc_mlp_apply.hip (inference inside a sweep, mask probe) and omc_nn_epoch.hip (epoch order):
//   * the transposed MFMA layout: accumulator register <-> hidden unit (unit_of), the swizzled LDS staging patches
//     (st_idx, StageOfs), the float32 MFMA wrapper;
//   * ReLU + inverted dropout for every register layout in use (relu_dropout, _1, _n, _t, _q16);
//   * the keyed epoch permutation (Shuffle, shuffle_index, make_shuffle);
//   * the flat parameter layout (mlp_params_of) and the gradient partial stride (tile_pstride);
//   * MlpNet -> MlpStepArgs / MlpAdamArgs (mlp_step_args, mlp_adam_args): host and device run the same conversions;
//   * the Adam update bodies;
//   * dispatch_hl: (hidden, layers) -> template arguments.
#pragma once
#include "omc_device.h"
#include "omc_kernels.h"

#include <cmath>
#include <type_traits>

namespace omc {

namespace {

constexpr int kH = 64;                 // hidden width of the workgroup trainer and of the local-vol network
constexpr int kLdW1 = 9, kLdW2 = 65;   // LDS leading dimensions (odd: conflict-free column walks)
// Staging patches are [unit][32 rows] without padding; the row index is XOR-swizzled per unit in
// units of 4 rows, so that the 16-byte row-quad reads of 16 consecutive units fall on 16 different
// bank groups and a quad stays contiguous.  (The last hidden layer's patch holds H, not dZ: the
// reading lane rebuilds dZ = [H > 0] wo dout / keep from it and gets the output-weight gradient
// from the same values, which saves the 32 per-lane accumulators a register-side sum would need.)
__device__ __forceinline__ int st_idx(int unit, int row) { return unit * 32 + (row ^ (((unit >> 1) & 7) << 2)); }
// The two access patterns of the trainers that stage through such patches, written so that every address is one of four per-lane
// registers plus a compile-time offset (an XOR with a lane-dependent value cannot be folded into
// the instruction's immediate offset; left to itself hipcc keeps ~100 separate addresses live):
//   write: unit = unit_of(mt, r, h), row = c        -> 32*unit_const(mt, r) + wr[((r >> 2) & 1) * 2 + ((r >> 1) & 1)]
//   read : unit = c (+32), rows 16h + 4q .. + 3     -> 32*32*(unit >= 32) + rd[q]
struct StageOfs { int wr[4], rd[4]; };
__device__ __forceinline__ StageOfs stage_offsets(int c, int h)
{
    StageOfs o;
    // swizzle of unit_of(mt, r, h): ((unit >> 1) & 7) = 4*((r >> 2) & 1) ^ 2*h ^ ((r >> 1) & 1)
#pragma unroll
    for (int v = 0; v < 4; ++v) o.wr[v] = 128 * h + (c ^ (((4 * (v >> 1)) ^ (2 * h) ^ (v & 1)) << 2));
#pragma unroll
    for (int q = 0; q < 4; ++q) o.rd[q] = c * 32 + ((16 * h + 4 * q) ^ (((c >> 1) & 7) << 2));
    return o;
}
// offset of unit_of(mt, r, h) without its h term (that one is in StageOfs::wr)
__device__ __forceinline__ constexpr int unit_base(int mt, int r) { return 32 * (32 * mt + (r >> 2) * 8 + (r & 3)); }
__device__ __forceinline__ constexpr int wr_sel(int r) { return ((r >> 2) & 1) * 2 + ((r >> 1) & 1); }

typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v4f16 __attribute__((ext_vector_type(4)));  // accumulator of the 16x16x4 MFMA (16-row tiles)

// hidden unit held by accumulator register r of 32x32 tile mt in half-wave h
__device__ __forceinline__ int unit_of(int mt, int r, int h) { return 32 * mt + (r >> 2) * 8 + 4 * h + (r & 3); }

__device__ __forceinline__ v16f mfma(float a, float b, v16f c)
{
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ void wave_sync_lds()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------ ReLU + inverted dropout
// One function per register layout; the tags and the unit maps of their callers are restated by oracle/dropout.py.
// ReLU + inverted dropout on one layer's pre-activations (32 per lane), in place.
// One Philox block per (row, half-wave, layer, step) seeds two multiply-with-carry streams
// (x <- a * lo32(x) + hi32(x): one v_mad_u64_u32 per 32 bits); 16 bits per unit, kept if
// below keep16.
// SCALE = false leaves the 1 / keep factor to the caller (the trainer folds it into the next
// layer's weights).
template <bool SCALE>
__device__ __forceinline__ void relu_dropout(v16f (&z)[2], uint32_t row, uint32_t step, uint32_t tag,
                                             uint32_t keep16, float inv_keep, uint32_t k0, uint32_t k1)
{
    if (keep16 >= 65536u) {  // no dropout (uniform branch)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) z[mt][r] = fmaxf(z[mt][r], 0.0f);
        return;
    }
    const U4 o = philox4x32_10(row, step, tag, 0x4d4c5031u, k0, k1);
    uint64_t st[2] = {((uint64_t)o.x << 32) | (o.y | 1u), ((uint64_t)o.z << 32) | (o.w | 1u)};
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
            st[mt] = (uint64_t)4294957665u * (uint32_t)st[mt] + (st[mt] >> 32);
            const uint32_t w = (uint32_t)st[mt];
            const float v0 = z[mt][e], v1 = z[mt][e + 1];
            z[mt][e] = (v0 > 0.0f && (w & 0xffffu) < keep16) ? (SCALE ? v0 * inv_keep : v0) : 0.0f;
            z[mt][e + 1] = (v1 > 0.0f && (w >> 16) < keep16) ? (SCALE ? v1 * inv_keep : v1) : 0.0f;
        }
    }
}

// ReLU + inverted dropout on ONE 32-unit tile's pre-activations (16 per lane), in place; same bit budget as
// relu_dropout (16 bits per unit from a multiply-with-carry stream seeded by one Philox block)
__device__ __forceinline__ void relu_dropout_1(v16f& z, uint32_t row, uint32_t step, uint32_t tag, uint32_t keep16,
                                               float inv_keep, uint32_t k0, uint32_t k1)
{
    if (keep16 >= 65536u) {
#pragma unroll
        for (int r = 0; r < 16; ++r) z[r] = fmaxf(z[r], 0.0f);
        return;
    }
    const U4 o = philox4x32_10(row, step, tag, 0x4d4c5134u, k0, k1);
    uint64_t st = ((uint64_t)(o.x ^ o.z) << 32) | ((o.y ^ o.w) | 1u);
#pragma unroll
    for (int e = 0; e < 16; e += 2) {
        st = (uint64_t)4294957665u * (uint32_t)st + (st >> 32);
        const uint32_t w = (uint32_t)st;
        const float v0 = z[e], v1 = z[e + 1];
        z[e] = (v0 > 0.0f && (w & 0xffffu) < keep16) ? v0 * inv_keep : 0.0f;
        z[e + 1] = (v1 > 0.0f && (w >> 16) < keep16) ? v1 * inv_keep : 0.0f;
    }
}

// ReLU + inverted dropout over NT 32-unit tiles; one Philox block seeds the two streams of a
// tile pair.
template <int NT>
__device__ __forceinline__ void relu_dropout_n(v16f (&z)[NT], uint32_t row, uint32_t step, uint32_t tag,
                                               uint32_t keep16, float inv_keep, uint32_t k0, uint32_t k1)
{
    if constexpr (NT == 1) {  // 32 hidden units: one tile, no partner -- the single-stream generator (relu_dropout_1)
        relu_dropout_1(z[0], row, step, tag, keep16, inv_keep, k0, k1);
        return;
    }
#pragma unroll
    for (int p = 0; p + 1 < NT; p += 2) {
        v16f pair[2] = {z[p], z[p + 1]};
        relu_dropout<true>(pair, row, step, tag + 0x1000u * (uint32_t)p, keep16, inv_keep, k0, k1);
        z[p] = pair[0];
        z[p + 1] = pair[1];
    }
}

// the tile-per-wave trainer's NT tiles, pair by pair
template <int NT, bool SCALE>
__device__ __forceinline__ void relu_dropout_t(v16f (&z)[NT], uint32_t row, uint32_t step, uint32_t tag,
                                               uint32_t keep16, float inv_keep, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int p = 0; p < NT; p += 2) {
        v16f pair[2] = {z[p], z[p + 1]};
        relu_dropout<SCALE>(pair, row, step, tag + 0x1000u * (uint32_t)p, keep16, inv_keep, k0, k1);
        z[p] = pair[0];
        z[p + 1] = pair[1];
    }
}

// ReLU + inverted dropout on a lane's eight consecutive units (z[ub][r] <-> unit offset e = 2 r + ub): 16 bits per unit
// straight from one Philox block -- word e / 2, half e % 2.  tag = 0x100 * (layer + 1) + (first unit / 8).
__device__ __forceinline__ void relu_dropout_q16(v4f16 (&z)[2], uint32_t row, uint32_t step, uint32_t tag, uint32_t keep16,
                                                 float inv_keep, uint32_t k0, uint32_t k1)
{
    if (keep16 >= 65536u) {
#pragma unroll
        for (int ub = 0; ub < 2; ++ub)
#pragma unroll
            for (int r = 0; r < 4; ++r) z[ub][r] = fmaxf(z[ub][r], 0.0f);
        return;
    }
    const U4 o = philox4x32_10(row, step, tag, 0x4d4c5138u, k0, k1);
    const uint32_t wd[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float v0 = z[0][r], v1 = z[1][r];
        z[0][r] = (v0 > 0.0f && (wd[r] & 0xffffu) < keep16) ? v0 * inv_keep : 0.0f;
        z[1][r] = (v1 > 0.0f && (wd[r] >> 16) < keep16) ? v1 * inv_keep : 0.0f;
    }
}

// ------------------------------------------------------------------ epoch order
// Pseudo-random permutation of [0, n): a 4-round Feistel network on ceil(log2 n) bits (the two
// halves may differ by one bit; an even number of rounds restores their order) with
// cycle-walking back into range.  Replaces randperm + gather: the kernel reads row perm(i).
struct Shuffle {
    uint64_t n;
    uint32_t abits, bbits;  // left / right half widths, abits + bbits = ceil(log2 n) (>= 2)
    uint32_t key[4];
    int on;
};

__device__ __forceinline__ uint32_t mix32(uint32_t x)
{
    x *= 0x9E3779B1u;
    x ^= x >> 15;
    x *= 0x85EBCA77u;
    x ^= x >> 13;
    return x;
}

__device__ __forceinline__ uint64_t shuffle_index(const Shuffle& s, uint64_t i)
{
    if (!s.on) return i;
    const uint32_t ma = (1u << s.abits) - 1u, mb = (1u << s.bbits) - 1u;  // widths <= 31
    do {
        uint32_t L = (uint32_t)(i >> s.bbits) & ma, R = (uint32_t)i & mb;
        // (L:a, R:b) -> (R:b, L ^ F(R):a) -> ... ; after 4 rounds the widths are (a, b) again
        uint32_t t;
        t = L ^ (mix32(R ^ s.key[0]) & ma); L = R; R = t;  // now L:b R:a
        t = L ^ (mix32(R ^ s.key[1]) & mb); L = R; R = t;  // now L:a R:b
        t = L ^ (mix32(R ^ s.key[2]) & ma); L = R; R = t;
        t = L ^ (mix32(R ^ s.key[3]) & mb); L = R; R = t;
        i = ((uint64_t)L << s.bbits) | R;
    } while (i >= s.n);
    return i;
}

// (host) the permutation of an epoch of n rows; key 0: storage order
inline Shuffle make_shuffle(int64_t n, uint64_t key)
{
    Shuffle sh;
    sh.n = (uint64_t)n;
    sh.on = (key != 0 && n > 1) ? 1 : 0;
    uint32_t bits = 2;
    while (bits < 62 && (1ull << bits) < sh.n) ++bits;
    sh.abits = bits / 2;
    sh.bbits = bits - sh.abits;
    for (int i = 0; i < 4; ++i) {  // splitmix64 of the key -> round keys
        uint64_t z = key + 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        sh.key[i] = (uint32_t)((z ^ (z >> 31)) >> 16);
    }
    return sh;
}

// ------------------------------------------------------------------ parameters, one optimizer step
// Flat parameter layout for any (H hidden units, L hidden layers): W1|b1 as [H][8], then for
// every further hidden layer its weights [H][H] and bias [H], then the output weights [H] and
// bias [1].
__host__ __device__ constexpr int mlp_params_of(int H, int L) { return H * 8 + (L - 1) * (H * H + H) + H + 1; }
// floats of one gradient partial of the tile trainers: the parameters + the loss slot, padded to 64
__host__ __device__ constexpr int tile_pstride(int H, int L) { return (mlp_params_of(H, L) + 1 + 63) / 64 * 64; }

// keep threshold on 16 random bits (65536: no dropout) and the 1 / keep of inverted dropout
struct DropKeep { uint32_t keep16; float inv_keep; };
inline DropKeep dropout_keep(double dropout)
{
    const uint32_t keep16 = dropout > 0.0 ? (uint32_t)llround((1.0 - dropout) * 65536.0) : 65536u;
    return {keep16, keep16 >= 65536u ? 1.0f : (float)(65536.0 / (double)keep16)};
}

// The forward / backward kernel's view of one optimizer step; all four trainers take this block.
struct MlpStepArgs {
    const float* data;    // [n][8]: 7 normalised features + normalised target (the whole epoch)
    const float* params;  // canonical layout, mlp_params_of(H, L)
    const float* wt;      // (L-1) x [H][H]: connection j transposed, wt_j[k][i] = W_j[i][k] (not read by mlp_train_kernel)
    float* partial;       // [partials][pstride]: gradient sums + batch loss
    int64_t row0, nrows;  // this step's minibatch = epoch positions row0 .. row0 + nrows
    Shuffle shuf;         // epoch position -> stored row
    int ntiles, pstride;
    float two_over_b, inv_keep;
    uint32_t keep16, step, k0, k1;
    // sharded training (omc_mlp_train_epoch_sharded): dropout key of local row i of this step = its position in the
    // GLOBAL minibatch (so every rank draws the masks of the unsharded run); null: the row's own position
    const uint32_t* drop_pos;
};

struct MlpAdamArgs {
    float* params;
    float* m;
    float* v;
    const float* partial;
    double* loss_acc;  // running sum of batch-mean losses of the epoch
    int nparts, nparams, stride;  // the loss slot is index nparams
    float inv_b, lr_t, inv_sqrt_bc2, beta1, beta2, eps, wd;
    float* wt;  // optional transposed copies of the connections (the tile trainers), else null
    int H, L;
};

// One network in training: what stays the same from step to step.  The host loop makes one from its MlpTrainPlan
// (omc_mlp.hip), the side-by-side kernels read one per problem from their table (omc_mlp_batch.hip); both get a step's
// two argument blocks from the two functions below, so the float conversions cannot drift apart (the IEEE double
// division / square root on the device round like the host's) and a net trained in a batch ends with the bits of its
// own call.
struct MlpNet {
    const float* data;
    float* params;
    float* m;
    float* v;
    float* partial;
    float* wt;  // null: the trainer keeps no transposed connections (mlp_train_kernel)
    double* loss_acc;
    double lr, beta1, beta2, eps, wd;
    Shuffle shuf;
    uint32_t keep16, k0, k1;
    float inv_keep;
    int pstride;
};

inline MlpNet mlp_net(const float* data, float* params, float* m, float* v, float* partial, float* wt, double* loss_acc,
                      double lr, double beta1, double beta2, double eps, double wd, const Shuffle& shuf, double dropout,
                      uint64_t seed, int pstride)
{
    const DropKeep k = dropout_keep(dropout);
    return {data, params, m, v, partial, wt, loss_acc, lr, beta1, beta2, eps, wd, shuf,
            k.keep16, (uint32_t)seed, (uint32_t)(seed >> 32), k.inv_keep, pstride};
}

// Optimizer step number `step` (1-based) on `local` rows from epoch position row0, in tiles of `tile_rows`; the
// minibatch has `global` rows over all ranks (= local unless sharded).
__host__ __device__ __forceinline__ MlpStepArgs mlp_step_args(const MlpNet& n, int64_t row0, int64_t local, int64_t global,
                                                              int tile_rows, int64_t step)
{
    MlpStepArgs a;
    a.data = n.data;
    a.params = n.params;
    a.wt = n.wt;
    a.partial = n.partial;
    a.row0 = row0;
    a.nrows = local;
    a.shuf = n.shuf;
    a.ntiles = (int)((local + tile_rows - 1) / tile_rows);
    a.pstride = n.pstride;
    a.two_over_b = (float)(2.0 / (double)global);
    a.keep16 = n.keep16;
    a.inv_keep = n.inv_keep;
    a.step = (uint32_t)step;
    a.k0 = n.k0;
    a.k1 = n.k1;
    a.drop_pos = nullptr;
    return a;
}

// The Adam launch that follows: `nparts` partials of the step; bc1 / bc2 = 1 - beta^step (libm pow on the host: the
// batch kernels read them from host-made tables).
__host__ __device__ __forceinline__ MlpAdamArgs mlp_adam_args(const MlpNet& n, int nparts, int H, int L, int64_t global,
                                                              double bc1, double bc2)
{
    MlpAdamArgs b;
    b.params = n.params;
    b.m = n.m;
    b.v = n.v;
    b.partial = n.partial;
    b.loss_acc = n.loss_acc;
    b.nparts = nparts;
    b.nparams = mlp_params_of(H, L);
    b.stride = n.pstride;
    b.wt = n.wt; b.H = H; b.L = L;
    b.inv_b = (float)(1.0 / (double)global);
    b.lr_t = (float)(n.lr / bc1);
    b.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    b.beta1 = (float)n.beta1;
    b.beta2 = (float)n.beta2;
    b.eps = (float)n.eps;
    b.wd = (float)n.wd;
    return b;
}

// ------------------------------------------------------------------ Adam
// Parameter p (value w0, moments m0, v0) once its gradient sum g is known: weight decay, moments, step, and the
// transposed mirror of a connection weight.
__device__ __forceinline__ void mlp_adam_update(const MlpAdamArgs& a, const int p, float g, const float w0, const float m0,
                                                const float v0)
{
    g = __builtin_fmaf(a.wd, w0, g);
    const float m = __builtin_fmaf(a.beta1, m0, (1.0f - a.beta1) * g);
    const float v = __builtin_fmaf(a.beta2, v0, (1.0f - a.beta2) * g * g);
    a.m[p] = m;
    a.v[p] = v;
    const float denom = __builtin_amdgcn_sqrtf(v) * a.inv_sqrt_bc2 + a.eps;
    const float w1 = w0 - a.lr_t * (m / denom);
    a.params[p] = w1;
    if (a.wt) {
        const int conn = a.H * a.H + a.H, q = p - a.H * 8;
        if (q >= 0 && q < (a.L - 1) * conn) {
            const int jc = q / conn, rem = q - jc * conn;
            if (rem < a.H * a.H) {
                const int i = rem / a.H, k = rem - i * a.H;
                a.wt[(size_t)jc * a.H * a.H + (size_t)k * a.H + i] = w1;
            }
        }
    }
}

// 16 parameters per workgroup, 16 threads per parameter: thread (slice, j) sums partials
// slice, slice + 16, ... of parameter j (independent loads, all in flight together), the 16 slice
// sums are added in slice order through LDS, thread (0, j) applies Adam.
// (Measured in round 4: 64 parameters per workgroup -- 256-byte reads of a partial -- takes the same 5.0 us at 256
// partials; the kernel is bound by the latency of its 16 loads per thread, not by their coalescing.)
__device__ __forceinline__ void mlp_adam_body(const MlpAdamArgs& a)
{
    __shared__ float red[16][17];
    const int j = threadIdx.x & 15, slice = threadIdx.x >> 4;
    const int p = blockIdx.x * 16 + j;
    // the parameter and its moments travel together with the partials (one memory latency per launch, not two)
    float w0 = 0.0f, m0 = 0.0f, v0 = 0.0f;
    if (slice == 0 && p < a.nparams) {
        w0 = a.params[p];
        m0 = a.m[p];
        v0 = a.v[p];
    }
    float g = 0.0f;
    if (p <= a.nparams) {
#pragma unroll 16
        for (int w = slice; w < a.nparts; w += 16) g += a.partial[(size_t)w * a.stride + p];
    }
    red[slice][j] = g;
    __syncthreads();
    if (slice != 0 || p > a.nparams) return;
    g = 0.0f;
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) g += red[s2][j];
    if (p == a.nparams) {  // the loss slot
        *a.loss_acc += (double)g * (double)a.inv_b;
        return;
    }
    mlp_adam_update(a, p, g, w0, m0, v0);
}

// The same update with ONE THREAD per parameter (256 parameters per workgroup): for the batched launches, where a
// workgroup of mlp_adam_body per 16 parameters and problem means tens of thousands of nearly empty workgroups.  The
// float additions are those of mlp_adam_body in the same order -- slice sums g_s = partial[s] + partial[s + 16] + ...
// (from 0), then g_0 + g_1 + ... + g_15 (from 0) -- so the parameters come out bit for bit the same.
__device__ __forceinline__ void mlp_adam_body_flat(const MlpAdamArgs& a, const int p)
{
    if (p > a.nparams) return;
    float g = 0.0f;
#pragma unroll 1
    for (int s0 = 0; s0 < 16; ++s0) {
        float gs = 0.0f;
        for (int w = s0; w < a.nparts; w += 16) gs += a.partial[(size_t)w * a.stride + p];
        g += gs;
    }
    if (p == a.nparams) {  // the loss slot
        *a.loss_acc += (double)g * (double)a.inv_b;
        return;
    }
    mlp_adam_update(a, p, g, a.params[p], a.m[p], a.v[p]);
}

// ------------------------------------------------------------------ (hidden, layers) -> template arguments
// f(std::integral_constant<int, H>{}[, std::integral_constant<int, L>{}]) for hidden in {32, 64, 128} and layers in
// {2, 3}: the shapes some kernel here is built for.  A call site that covers fewer says so with `if constexpr` in
// its lambda (and so instantiates no kernel for the others).  Anything else: hipErrorInvalidValue.
template <class F>
hipError_t dispatch_h(int hidden, F&& f)
{
    if (hidden == 32) return f(std::integral_constant<int, 32>{});
    if (hidden == 64) return f(std::integral_constant<int, 64>{});
    if (hidden == 128) return f(std::integral_constant<int, 128>{});
    return hipErrorInvalidValue;
}
template <class F>
hipError_t dispatch_hl(int hidden, int layers, F&& f)
{
    return dispatch_h(hidden, [&](auto H) -> hipError_t {
        if (layers == 2) return f(H, std::integral_constant<int, 2>{});
        if (layers == 3) return f(H, std::integral_constant<int, 3>{});
        return hipErrorInvalidValue;
    });
}

}  // namespace

}  // namespace omc
