// omc_mlp_quad_dev.h -- the two tile-per-workgroup training steps as device functions: mlp_train_quad_body (32-row
// tiles, any of 32 / 64 / 128 units) and mlp_train_q16_body (16-row tiles, 64 / 128 units).  One call = forward,
// backward and the gradient partial of ONE tile of one network.  omc_mlp.hip wraps them into the single-network
// kernels, omc_mlp_batch.hip into the side-by-side ones; a network therefore gets the same bits either way.
#pragma once
#include "omc_mlp_dev.h"

namespace omc {

namespace {

// ------------------------------------------------------------------ tile-per-workgroup trainer
// Small minibatches -- the reference's own batch of 256 rows is 8 tiles -- leave the tile-per-wave kernel
// with 8 waves on the whole chip, each running ~390 float32 MFMAs of 64 cycles in sequence (65 us per
// step at 3 x 128).  Here one 32-row tile is a WORKGROUP of W = H / 32 waves, one per SIMD: wave w owns
// units 32w .. 32w + 31 of every hidden layer, so each wave issues a quarter of the MFMAs and the four
// SIMDs of the CU work on the tile together.  A layer's activations (and, going back, dZ) are exchanged
// through LDS in the swizzled [unit][32 rows] layout of the other trainers: the forward / dH products
// read them as B operands one value per lane ([unit][row c]: a permutation of a row, conflict-free),
// the weight-gradient products as 16-byte row quads.  Weights come from global memory / L2 (canonical
// layout for W^T dZ, the transposed copy for the forward products: both coalesced over the 32 units a
// wave owns), one group of 16 k-steps ahead of the MFMAs that use them.  Every gradient entry is written
// exactly once per tile (no accumulation across launches): ntiles <= kMlpMaxGroups workgroups, one
// partial each, summed by the Adam kernel in index order -- bitwise reproducible like the others.
template <int H, int L>
__device__ __forceinline__ void mlp_train_quad_body(const MlpStepArgs& a, const int tile)
{
    constexpr int W = H / 32, NP = mlp_params_of(H, L), CONN = H * H + H;
    __shared__ float sAct[L][H * 32];  // H_j, swizzled [unit][32 rows]
    __shared__ float sDz[H * 32];      // dZ_j of the layer being back-propagated
    __shared__ float sX[8 * 32];       // inputs [in][row] (row 7 = the bias column of ones)
    __shared__ float sO[W * 32];       // per-wave partial outputs
    __shared__ float sD[32];           // d(loss)/d(out) per row
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    auto rho = [&](int r) { return (r >> 2) * 8 + 4 * h + (r & 3); };  // tile row of accumulator register r
    if (tile >= a.ntiles) return;
    float* out = a.partial + (size_t)tile * a.pstride;
    const float* Wo = a.params + H * 8 + (L - 1) * CONN;
    const int64_t row = (int64_t)tile * 32 + c;
    const uint32_t drow = (a.drop_pos && a.keep16 < 65536u && row < a.nrows) ? a.drop_pos[row] : (uint32_t)row;
    const bool live = row < a.nrows;
    float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live) x = reinterpret_cast<const float4*>(a.data + shuffle_index(a.shuf, (uint64_t)(a.row0 + row)) * 8)[h];
    float y = x.w;
    if (h == 1) x.w = 1.0f;
    y = __shfl(y, c + 32, 64);
    if (w == 0) {
        sX[(4 * h + 0) * 32 + c] = x.x;
        sX[(4 * h + 1) * 32 + c] = x.y;
        sX[(4 * h + 2) * 32 + c] = x.z;
        sX[(4 * h + 3) * 32 + c] = x.w;
    }

    // ---- layer 0: own 32 units x 8 inputs
    v16f hreg[L];
    {
        v16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        const float4 wv = *reinterpret_cast<const float4*>(a.params + (32 * w + c) * 8 + 4 * h);
        acc = mfma(wv.x, x.x, acc);
        acc = mfma(wv.y, x.y, acc);
        acc = mfma(wv.z, x.z, acc);
        acc = mfma(wv.w, x.w, acc);
        relu_dropout_1(acc, drow, a.step, 0x100u + 0x10u * (uint32_t)w + (uint32_t)h, a.keep16, a.inv_keep, a.k0,
                       a.k1);
        hreg[0] = acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sAct[0][st_idx(32 * w + rho(r), c)] = acc[r];
    }
    __syncthreads();

    // 16 k-steps of one 32-unit block kt: A from global memory (row of `Wsrc` = k unit, 32 own units contiguous),
    // B from the swizzled LDS image `Bsrc`; the next block's weights are requested before this block's MFMAs
    auto product = [&](const float* Wsrc, const float* Bsrc, v16f acc) {
        float wa[2][16];
        auto fetch = [&](int kt, float (&dst)[16]) {
#pragma unroll
            for (int s2 = 0; s2 < 16; ++s2) dst[s2] = Wsrc[(size_t)(32 * kt + rho(s2)) * H + 32 * w + c];
        };
        fetch(0, wa[0]);
#pragma unroll
        for (int kt = 0; kt < W; ++kt) {
            if (kt + 1 < W) fetch(kt + 1, wa[(kt + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            float b[16];
#pragma unroll
            for (int s2 = 0; s2 < 16; ++s2) b[s2] = Bsrc[st_idx(32 * kt + rho(s2), c)];
#pragma unroll
            for (int s2 = 0; s2 < 16; ++s2) acc = mfma(wa[kt & 1][s2], b[s2], acc);
        }
        return acc;
    };

    // ---- layers 1 .. L-1
#pragma unroll
    for (int j = 1; j < L; ++j) {
        const float* bj = a.params + H * 8 + (size_t)(j - 1) * CONN + H * H;
        v16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bj[32 * w + rho(r)];
        acc = product(a.wt + (size_t)(j - 1) * H * H, sAct[j - 1], acc);
        relu_dropout_1(acc, drow, a.step, 0x100u * (uint32_t)(j + 1) + 0x10u * (uint32_t)w + (uint32_t)h, a.keep16,
                       a.inv_keep, a.k0, a.k1);
        hreg[j] = acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sAct[j][st_idx(32 * w + rho(r), c)] = acc[r];
        __syncthreads();
    }

    // ---- output, loss, d(loss)/d(out): every wave ends with the same numbers
    float wo[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) wo[r] = Wo[32 * w + rho(r)];
    {
        float o = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) o = __builtin_fmaf(wo[r], hreg[L - 1][r], o);
        o += __shfl_xor(o, 32, 64);
        if (h == 0) sO[w * 32 + c] = o;
    }
    __syncthreads();
    float o = Wo[H];
#pragma unroll
    for (int ww = 0; ww < W; ++ww) o += sO[ww * 32 + c];
    const float diff = live ? o - y : 0.0f;
    const float dout = diff * a.two_over_b;
    if (w == 0 && h == 0) sD[c] = dout;
    v16f dz;
#pragma unroll
    for (int r = 0; r < 16; ++r) dz[r] = hreg[L - 1][r] > 0.0f ? wo[r] * dout * a.inv_keep : 0.0f;
    __syncthreads();

    // swizzled 16-byte read of rows 16h + 4q .. + 3 of `unit`
    auto quad = [&](const float* base, int unit, int q) {
        return *reinterpret_cast<const float4*>(base + unit * 32 + ((16 * h + 4 * q) ^ (((unit >> 1) & 7) << 2)));
    };

    // output-weight gradient of the own units: sum over rows of dout * H_{L-1}
    {
        float gws = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 e = quad(sAct[L - 1], 32 * w + c, q);
            const float4 d = *reinterpret_cast<const float4*>(sD + 16 * h + 4 * q);
            gws = __builtin_fmaf(e.x, d.x, gws);
            gws = __builtin_fmaf(e.y, d.y, gws);
            gws = __builtin_fmaf(e.z, d.z, gws);
            gws = __builtin_fmaf(e.w, d.w, gws);
        }
        gws += __shfl_xor(gws, 32, 64);
        if (h == 0) out[H * 8 + (L - 1) * CONN + 32 * w + c] = gws;
    }

#pragma unroll
    for (int j = L - 1; j >= 1; --j) {
        const float* Wj = a.params + H * 8 + (size_t)(j - 1) * CONN;
        float* gWj = out + H * 8 + (size_t)(j - 1) * CONN;
#pragma unroll
        for (int r = 0; r < 16; ++r) sDz[st_idx(32 * w + rho(r), c)] = dz[r];
        __syncthreads();
        // ---- gW_j rows = own units, all H columns: contraction over the 32 batch rows
        {
            v16f acc[W];
#pragma unroll
            for (int nt = 0; nt < W; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[nt][r] = 0.0f;
            float gbs = 0.0f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 ea = quad(sDz, 32 * w + c, q);
                const float av[4] = {ea.x, ea.y, ea.z, ea.w};
                float bv[W][4];
#pragma unroll
                for (int nt = 0; nt < W; ++nt) {
                    const float4 eb = quad(sAct[j - 1], 32 * nt + c, q);
                    bv[nt][0] = eb.x; bv[nt][1] = eb.y; bv[nt][2] = eb.z; bv[nt][3] = eb.w;
                }
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    gbs += av[jj];
#pragma unroll
                    for (int nt = 0; nt < W; ++nt) acc[nt] = mfma(av[jj], bv[nt][jj], acc[nt]);
                }
            }
#pragma unroll
            for (int nt = 0; nt < W; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) gWj[(size_t)(32 * w + rho(r)) * H + 32 * nt + c] = acc[nt][r];
            gbs += __shfl_xor(gbs, 32, 64);
            if (h == 0) gWj[H * H + 32 * w + c] = gbs;
        }
        // ---- dH_{j-1} of the own units = W_j^T dZ_j, then through the ReLU / dropout mask of H_{j-1}
        {
            v16f d;
#pragma unroll
            for (int r = 0; r < 16; ++r) d[r] = 0.0f;
            d = product(Wj, sDz, d);
#pragma unroll
            for (int r = 0; r < 16; ++r) dz[r] = hreg[j - 1][r] > 0.0f ? d[r] * a.inv_keep : 0.0f;
        }
        __syncthreads();  // every wave is done with sDz
    }

    // ---- gW1 (own units x 8 inputs, bias in column 7): 16 rows per half-wave on the vector unit
#pragma unroll
    for (int r = 0; r < 16; ++r) sDz[st_idx(32 * w + rho(r), c)] = dz[r];
    __syncthreads();
    {
        float g[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 e = quad(sDz, 32 * w + c, q);
            const float ev[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
            for (int in = 0; in < 8; ++in) {
                const float4 xv = *reinterpret_cast<const float4*>(sX + in * 32 + 16 * h + 4 * q);
                g[in] = __builtin_fmaf(ev[0], xv.x, g[in]);
                g[in] = __builtin_fmaf(ev[1], xv.y, g[in]);
                g[in] = __builtin_fmaf(ev[2], xv.z, g[in]);
                g[in] = __builtin_fmaf(ev[3], xv.w, g[in]);
            }
        }
#pragma unroll
        for (int in = 0; in < 8; ++in) g[in] += __shfl_xor(g[in], 32, 64);
        if (h == 0) {
            float4* po = reinterpret_cast<float4*>(out + (32 * w + c) * 8);
            po[0] = make_float4(g[0], g[1], g[2], g[3]);
            po[1] = make_float4(g[4], g[5], g[6], g[7]);
        }
    }
    if (w == 0) {
        float gbo = h == 0 ? dout : 0.0f, loss = h == 0 ? diff * diff : 0.0f;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            gbo += __shfl_xor(gbo, m, 64);
            loss += __shfl_xor(loss, m, 64);
        }
        if (lane == 0) {
            out[NP - 1] = gbo;
            out[NP] = loss;
        }
    }
}

// ------------------------------------------------------------------ 16-row tiles: the reference's own minibatch
// The reference trains on minibatches of min(256, R) rows (options_model_3.py:574): 22,000 optimizer steps of 256 rows
// at its default call.  In 32-row tiles that is 8 workgroups on a 256-CU chip, each running ~390 float32 MFMAs of 64
// cycles behind one another and waiting for every block of weights to come back from L2 (round 5 profile: 23.7 us
// per step at 3 x 128, of which 10 us are MFMA issue).  This kernel halves the serial part and takes the weight
// fetches off the critical path:
//   * a workgroup owns a 16-row tile and runs v_mfma_f32_16x16x4_f32 (the same multiply-adds per cycle as 32x32x2):
//     twice the workgroups, half the MFMA cycles each;
//   * ALL A operands of a 128 x 128 product (64 registers per lane) are requested a whole product ahead -- the forward
//     products' at kernel entry, each backward product's as soon as the forward product that used the same registers
//     is done -- so a product never waits for L2 (one wave per SIMD: 512 registers are there);
//   * activations go through LDS in [k / 4][row][k % 4] order: the B operands of four k-steps are ONE 16-byte read.
// Wave w owns hidden units 32 w .. 32 w + 31 of every layer, as two 16-row MFMA blocks ub = 0, 1 holding the even and
// the odd units (output row m of block ub <-> unit 32 w + 2 m + ub: the two blocks' weights are one 8-byte load).
// After an MFMA lane (row j = lane % 16, g = lane / 16) holds, for its row, the EIGHT CONSECUTIVE units 32 w + 8 g + e,
// e = 2 r + ub (register r of block ub): dropout draws one Philox block (8 x 16 bits) per lane and layer.
// k-step (q, t) of a product contracts k = 16 q + 4 g + t in lane group g -- any order is fine as long as A and B agree.
__device__ __forceinline__ v4f16 mfma16(float a, float b, v4f16 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

template <int H, int L>
__device__ __forceinline__ void mlp_train_q16_body(const MlpStepArgs& a, const int tile)
{
    constexpr int W = H / 32, NP = mlp_params_of(H, L), CONN = H * H + H, NQ = H / 16, KS = H / 4;
    __shared__ __attribute__((aligned(16))) float sAct[L][H * 16];  // H_j, [k / 4][16 rows][k % 4]
    __shared__ __attribute__((aligned(16))) float sDz[H * 16];      // dZ_j of the layer being back-propagated, same order
    __shared__ float sX[8 * 16];                                    // inputs [in][row] (row 7 = the bias column of ones)
    __shared__ float sO[W * 16];                                    // per-wave partial outputs
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, g = lane >> 4;
    if (tile >= a.ntiles) return;
    float* out = a.partial + (size_t)tile * a.pstride;
    const float* Wo = a.params + H * 8 + (L - 1) * CONN;

    // A operands of one H x H product: row k of `src` is the contraction index, this wave's 32 columns 32 w + 2 j, + 1
    auto fetch_w = [&](const float* __restrict__ src, float2 (&dst)[KS]) {
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                dst[4 * q + t] = *reinterpret_cast<const float2*>(src + (size_t)(16 * q + 4 * g + t) * H + 32 * w + 2 * j);
            }
    };
    // acc[ub] += A (registers) x B (LDS image of the previous layer / of dZ)
    auto product = [&](const float2 (&wa)[KS], const float* Bsrc, v4f16 (&acc)[2]) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float4 b = *reinterpret_cast<const float4*>(Bsrc + (4 * q + g) * 64 + j * 4);
            const float bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                acc[0] = mfma16(wa[4 * q + t].x, bv[t], acc[0]);
                acc[1] = mfma16(wa[4 * q + t].y, bv[t], acc[1]);
            }
        }
    };
    // a lane's eight units of its row -> LDS in [k / 4][row][k % 4] order (two 16-byte stores)
    auto put = [&](float* dst, const v4f16 (&v)[2]) {
#pragma unroll
        for (int rh = 0; rh < 2; ++rh)
            *reinterpret_cast<float4*>(dst + (8 * w + 2 * g + rh) * 64 + j * 4) =
                make_float4(v[0][2 * rh], v[1][2 * rh], v[0][2 * rh + 1], v[1][2 * rh + 1]);
    };
    // units 32 w + 2 j, + 1 of an LDS image at row 4 s + g: the operand of the products that contract over the rows
    auto own_pair = [&](const float* src, int s2) {
        return *reinterpret_cast<const float2*>(src + (8 * w + (j >> 1)) * 64 + (4 * s2 + g) * 4 + 2 * (j & 1));
    };

    // ---- every small load first, then the big ones: loads return in order, and each of these would otherwise expose
    // one L2-miss latency on the step's critical path (the parameters were just rewritten by the Adam kernel)
    const int64_t row = (int64_t)tile * 16 + j;
    const bool live = row < a.nrows;
    float xa = 0.0f, xb = 0.0f;  // inputs g and 4 + g of the lane's row
    if (live) {
        const float* xr = a.data + shuffle_index(a.shuf, (uint64_t)(a.row0 + row)) * 8;
        xa = xr[g];
        xb = xr[4 + g];
    }
    const uint32_t drow = (a.drop_pos && a.keep16 < 65536u && live) ? a.drop_pos[row] : (uint32_t)row;
    float w1v[2][2];  // layer-0 weights of units 32 w + 2 j + ub, inputs g and 4 + g
#pragma unroll
    for (int ub = 0; ub < 2; ++ub) {
        const float* wr = a.params + (32 * w + 2 * j + ub) * 8 + g;
        w1v[ub][0] = wr[0];
        w1v[ub][1] = wr[4];
    }
    float4 bias[L > 1 ? L - 1 : 1][2];  // biases of the lane's eight units 32 w + 8 g .. + 7
#pragma unroll
    for (int l = 1; l < L; ++l) {
        const float* bj = a.params + H * 8 + (size_t)(l - 1) * CONN + H * H + 32 * w + 8 * g;
        bias[l - 1][0] = *reinterpret_cast<const float4*>(bj);
        bias[l - 1][1] = *reinterpret_cast<const float4*>(bj + 4);
    }
    const float4 wo0 = *reinterpret_cast<const float4*>(Wo + 32 * w + 8 * g),
                 wo1 = *reinterpret_cast<const float4*>(Wo + 32 * w + 8 * g + 4);
    const float bo = Wo[H];

    float2 wbuf[L - 1][KS];  // connection c: first its transposed copy (forward), then the canonical matrix (dH)
#pragma unroll
    for (int c = 0; c < L - 1; ++c) fetch_w(a.wt + (size_t)c * H * H, wbuf[c]);

    const float y = __shfl(xb, 48 + j, 64);  // column 7 is the target ...
    if (g == 3) xb = 1.0f;                   // ... and its slot carries the bias input
    if (w == 0) {
        sX[g * 16 + j] = xa;
        sX[(4 + g) * 16 + j] = xb;
    }

    // ---- layer 0: own 32 units x 8 inputs, k-steps s = 0, 1 <-> inputs 4 s + g
    v4f16 hreg[L][2];
    {
        v4f16 acc[2];
#pragma unroll
        for (int ub = 0; ub < 2; ++ub) {
            acc[ub] = v4f16{0.0f, 0.0f, 0.0f, 0.0f};
            acc[ub] = mfma16(w1v[ub][0], xa, acc[ub]);
            acc[ub] = mfma16(w1v[ub][1], xb, acc[ub]);
        }
        relu_dropout_q16(acc, drow, a.step, 0x100u + (uint32_t)(4 * w + g), a.keep16, a.inv_keep, a.k0, a.k1);
        hreg[0][0] = acc[0];
        hreg[0][1] = acc[1];
        put(sAct[0], acc);
    }
    __syncthreads();

    // ---- layers 1 .. L-1
#pragma unroll
    for (int l = 1; l < L; ++l) {
        const float4 b0 = bias[l - 1][0], b1 = bias[l - 1][1];
        v4f16 acc[2] = {v4f16{b0.x, b0.z, b1.x, b1.z}, v4f16{b0.y, b0.w, b1.y, b1.w}};  // unit offset e = 2 r + ub
        product(wbuf[l - 1], sAct[l - 1], acc);
        fetch_w(a.params + H * 8 + (size_t)(l - 1) * CONN, wbuf[l - 1]);  // the same connection, canonical: for dH
        relu_dropout_q16(acc, drow, a.step, 0x100u * (uint32_t)(l + 1) + (uint32_t)(4 * w + g), a.keep16, a.inv_keep,
                         a.k0, a.k1);
        hreg[l][0] = acc[0];
        hreg[l][1] = acc[1];
        put(sAct[l], acc);
        __syncthreads();
    }

    // ---- output, loss, d(loss)/d(out): every wave ends with the same numbers
    const float wo[2][4] = {{wo0.x, wo0.z, wo1.x, wo1.z}, {wo0.y, wo0.w, wo1.y, wo1.w}};  // wo[ub][r] <-> unit offset 2 r + ub
    {
        float o = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            o = __builtin_fmaf(wo[0][r], hreg[L - 1][0][r], o);
            o = __builtin_fmaf(wo[1][r], hreg[L - 1][1][r], o);
        }
        o += __shfl_xor(o, 16, 64);
        o += __shfl_xor(o, 32, 64);
        if (g == 0) sO[w * 16 + j] = o;
    }
    __syncthreads();
    float o = bo;
#pragma unroll
    for (int ww = 0; ww < W; ++ww) o += sO[ww * 16 + j];
    const float diff = live ? o - y : 0.0f;
    const float dout = diff * a.two_over_b;
    v4f16 dz[2];
#pragma unroll
    for (int ub = 0; ub < 2; ++ub)
#pragma unroll
        for (int r = 0; r < 4; ++r) dz[ub][r] = hreg[L - 1][ub][r] > 0.0f ? wo[ub][r] * dout * a.inv_keep : 0.0f;
    // output-weight gradient of the own units: sum over rows of dout * H_{L-1} as one more contraction over the rows
    // (A = dout of row 4 s + g for every output row, B = H_{L-1} of unit 32 w + 2 n + ub): every output row holds the sum
    {
        v4f16 acc[2] = {v4f16{0.0f, 0.0f, 0.0f, 0.0f}, v4f16{0.0f, 0.0f, 0.0f, 0.0f}};
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) {
            const float dv = __shfl(dout, 4 * s2 + g, 64);  // lanes 0 .. 15 hold the rows' values
            const float2 hv = own_pair(sAct[L - 1], s2);
            acc[0] = mfma16(dv, hv.x, acc[0]);
            acc[1] = mfma16(dv, hv.y, acc[1]);
        }
        if (g == 0) *reinterpret_cast<float2*>(out + H * 8 + (L - 1) * CONN + 32 * w + 2 * j) = make_float2(acc[0][0], acc[1][0]);
    }
#pragma unroll
    for (int l = L - 1; l >= 1; --l) {
        float* gWl = out + H * 8 + (size_t)(l - 1) * CONN;
        put(sDz, dz);
        __syncthreads();
        // ---- gW_l, transposed product: rows of the MFMA <-> columns k of gW_l (A = H_{l-1} of unit 16 kb + j), columns
        // <-> own units i = 32 w + 2 n + ub (B = dZ_l); contraction over the 16 rows, k-step s <-> rows 4 s + g.  A lane's
        // four registers are gW_l[i][16 kb + 4 g .. + 3]: one 16-byte store.  Block NQ has A = 1: the bias gradient.
        {
            // The column blocks in two halves: half as many accumulators live at a time (with the weights of two
            // connections in flight the kernel sits at the 256 registers that still let two workgroups share a CU --
            // what the side-by-side trainer of a curve's networks needs; every output element sums its four k-steps in
            // the same order either way).  Every LDS operand of a half is requested before its first MFMA (left to
            // itself hipcc puts each ds_read directly in front of the pair of MFMAs that uses it).
            float2 dv[4];
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) dv[s2] = own_pair(sDz, s2);
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                constexpr int NH = NQ / 2;
                v4f16 acc[2][NH + 1];
#pragma unroll
                for (int ub = 0; ub < 2; ++ub)
#pragma unroll
                    for (int kb = 0; kb <= NH; ++kb) acc[ub][kb] = v4f16{0.0f, 0.0f, 0.0f, 0.0f};
                float hv[4][NH];
#pragma unroll
                for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
                    for (int kb = 0; kb < NH; ++kb)
                        hv[s2][kb] = sAct[l - 1][(4 * (NH * half + kb) + (j >> 2)) * 64 + (4 * s2 + g) * 4 + (j & 3)];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s2 = 0; s2 < 4; ++s2) {
#pragma unroll
                    for (int kb = 0; kb < NH; ++kb) {
                        acc[0][kb] = mfma16(hv[s2][kb], dv[s2].x, acc[0][kb]);
                        acc[1][kb] = mfma16(hv[s2][kb], dv[s2].y, acc[1][kb]);
                    }
                    if (half == 1) {  // block NQ has A = 1: the bias gradient
                        acc[0][NH] = mfma16(1.0f, dv[s2].x, acc[0][NH]);
                        acc[1][NH] = mfma16(1.0f, dv[s2].y, acc[1][NH]);
                    }
                }
#pragma unroll
                for (int ub = 0; ub < 2; ++ub)
#pragma unroll
                    for (int kb = 0; kb < NH; ++kb)
                        *reinterpret_cast<float4*>(gWl + (size_t)(32 * w + 2 * j + ub) * H + 16 * (NH * half + kb) + 4 * g) =
                            make_float4(acc[ub][kb][0], acc[ub][kb][1], acc[ub][kb][2], acc[ub][kb][3]);
                if (half == 1 && g == 0)
                    *reinterpret_cast<float2*>(gWl + H * H + 32 * w + 2 * j) = make_float2(acc[0][NH][0], acc[1][NH][0]);
            }
        }
        // ---- dH_{l-1} of the own units = W_l^T dZ_l, then through the ReLU / dropout mask of H_{l-1}
        {
            v4f16 d[2] = {v4f16{0.0f, 0.0f, 0.0f, 0.0f}, v4f16{0.0f, 0.0f, 0.0f, 0.0f}};
            product(wbuf[l - 1], sDz, d);
#pragma unroll
            for (int ub = 0; ub < 2; ++ub)
#pragma unroll
                for (int r = 0; r < 4; ++r) dz[ub][r] = hreg[l - 1][ub][r] > 0.0f ? d[ub][r] * a.inv_keep : 0.0f;
        }
        __syncthreads();  // every wave is done with sDz
    }

    // ---- gW1 (own units x 8 inputs, bias in column 7): the same transposed contraction, MFMA rows = inputs
    put(sDz, dz);
    __syncthreads();
    {
        v4f16 acc[2] = {v4f16{0.0f, 0.0f, 0.0f, 0.0f}, v4f16{0.0f, 0.0f, 0.0f, 0.0f}};
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) {
            const float2 dv = own_pair(sDz, s2);
            const float xv = j < 8 ? sX[j * 16 + 4 * s2 + g] : 0.0f;
            acc[0] = mfma16(xv, dv.x, acc[0]);
            acc[1] = mfma16(xv, dv.y, acc[1]);
        }
        if (g < 2) {  // registers = inputs 4 g .. 4 g + 3 of unit 32 w + 2 j + ub
#pragma unroll
            for (int ub = 0; ub < 2; ++ub)
                *reinterpret_cast<float4*>(out + (32 * w + 2 * j + ub) * 8 + 4 * g) =
                    make_float4(acc[ub][0], acc[ub][1], acc[ub][2], acc[ub][3]);
        }
    }
    if (w == 0) {
        float gbo = g == 0 ? dout : 0.0f, loss = g == 0 ? diff * diff : 0.0f;
#pragma unroll
        for (int mk = 1; mk < 16; mk <<= 1) {
            gbo += __shfl_xor(gbo, mk, 64);
            loss += __shfl_xor(loss, mk, 64);
        }
        if (lane == 0) {
            out[NP - 1] = gbo;
            out[NP] = loss;
        }
    }
}

}  // namespace

}  // namespace omc
