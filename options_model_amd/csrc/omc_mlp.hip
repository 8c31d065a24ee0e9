// omc_mlp.hip -- training one continuation-value network (SingleLSMNet, options_model_3.py:85-103, 565-600: Linear /
// ReLU / Dropout stacks of 32, 64 or 128 units x 2 or 3 hidden layers, MSE, Adam with weight decay; SURVEY.md
// section 8 row f-1) as hand-written gfx950 kernels.  In this file:
//   * four forward + backward kernels, one per regime of (width, minibatch size) -- mlp_train_kernel (64 units, large
//     minibatches, weights in LDS), mlp_train_tile_kernel (one wave per 32-row tile), mlp_train_quad_kernel and
//     mlp_train_q16_kernel (one workgroup per 32- / 16-row tile; bodies in omc_mlp_quad_dev.h) -- and which one runs
//     when (mlp_train_kernel_choice);
//   * the gradient reduce + Adam kernel, and the three launches of a sharded step around the all-reduce;
//   * the host loop over an epoch's optimizer steps (run_steps, mlp_train_steps).
// Many networks side by side: omc_mlp_batch.hip.  Inference: omc_mlp_apply.hip.  Epoch order, sharding, feature
// statistics: omc_nn_epoch.hip.  Shared device code: omc_mlp_dev.h.
//
// Common to all four: the minibatch GEMMs run on the matrix cores in float32 (v_mfma_f32_32x32x2_f32 /
// _16x16x4_f32; the reference trains in float32).  Everything is kept TRANSPOSED -- activations are [hidden][row] --
// so that the accumulator layout of one layer (lane <-> batch row, registers <-> hidden units) is directly the B
// operand of the next layer's MFMA: the k-index of a matrix product may be walked in any order as long as A and B
// agree, and the order chosen here is the one the accumulator registers already have.  Only the weight-gradient
// products, which contract over the batch rows, need the operands turned around; they go through LDS.  Every
// kernel writes gradient partials that the Adam kernel sums in index order.  No atomics: a training run is bitwise
// reproducible.
#include "omc_mlp_quad_dev.h"

#include <algorithm>
#include <cstdlib>

namespace omc {

namespace {

// ------------------------------------------------------------------ workgroup trainer (64 units, weights in LDS)
// One wave owns a tile of 32 batch rows from load to weight gradients; a workgroup (4 waves, one per SIMD, up to
// 512 registers each) shares the weights in LDS.  Gradients accumulate in registers over all tiles of a wave, are
// summed over the workgroup in a fixed order and written as one partial per workgroup.
// sizes for L hidden layers of 64 units
__host__ __device__ constexpr int train_params(int L) { return mlp_params_of(kH, L); }
__host__ __device__ constexpr int g_stride(int L) { return (train_params(L) + 1 + 63) / 64 * 64; }
__host__ __device__ constexpr int lds_weights(int L) { return kH * kLdW1 + (L - 1) * (kH * kLdW2 + kH) + kH + 4; }
__host__ __device__ constexpr int lds_wave(int L) { return L * kH * 32 + 9 * 32; }  // L patches + X + dout row
__host__ __device__ constexpr int train_lds_floats(int L)
{
    return lds_weights(L) + 4 * lds_wave(L) > 4 * g_stride(L) ? lds_weights(L) + 4 * lds_wave(L) : 4 * g_stride(L);
}
static_assert(g_stride(2) == kMlpPartialStride2 && g_stride(3) == kMlpPartialStride3, "omc_kernels.h");
static_assert(train_lds_floats(3) * 4 <= 160 * 1024, "LDS of one CU");

// L hidden layers.  Connection j (j = 1 .. L-1) is the 64x64 matrix from hidden layer j-1 to j;
// patch j holds H_j until its weight-gradient product has read it, then dZ_j.
template <int L>
__global__ __launch_bounds__(256) void mlp_train_kernel(MlpStepArgs a)
{
    constexpr int kConn = kH * kLdW2 + kH;  // one staged connection: weights [64][65] + bias [64]
    extern __shared__ float lds[];
    float* sW1 = lds;
    float* sWc = sW1 + kH * kLdW1;            // (L-1) connections, pre-multiplied by 1 / keep
    float* sWo = sWc + (L - 1) * kConn;       // output weights (pre-multiplied) ...
    float* sBo = sWo + kH;                    // ... and bias
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, h = lane >> 5;
    float* patch = lds + lds_weights(L) + wave * lds_wave(L);  // [L][64][32]
    float* tX = patch + L * kH * 32;                           // [8][32] inputs + [32] d(loss)/d(out)

    const StageOfs so = stage_offsets(c, h);
    const int nwaves = gridDim.x * 4;
    auto fetch = [&](int tile) {
        const int64_t r = (int64_t)tile * 32 + c;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (tile < a.ntiles && r < a.nrows)
            v = reinterpret_cast<const float4*>(a.data + shuffle_index(a.shuf, (uint64_t)(a.row0 + r)) * 8)[h];
        return v;
    };
    float4 xnext = fetch(blockIdx.x * 4 + wave);  // travels while the weights are staged

    // Inverted dropout's 1 / keep is folded into the weights that consume the dropped activations
    // (connections and output weights are staged pre-multiplied), so activations carry the 0/1
    // mask only: with H' = mask * relu(Z), Ws = W / keep: Z_j = Ws H'_{j-1} + b, dZ_{j-1} =
    // [H'_{j-1} > 0] Ws^T dZ_j, and the gradients taken against H' (connections, output weights)
    // are multiplied by 1 / keep once, on the way out.
    // Every load of the staging is issued before the first LDS store (one global round trip for the whole parameter
    // block instead of one per pair of loop iterations: the launch's fixed cost, 11.9 -> see DESIGN.md section 6).
    {
        constexpr int kTail = kH * 8 + (L - 1) * (kH * kH + kH);  // output weights [kH], then the output bias
        float w1v[2], wcv[L - 1][16], bcv[L - 1];
#pragma unroll
        for (int k = 0; k < 2; ++k) w1v[k] = a.params[tid + 256 * k];  // kH * 8 = 512
#pragma unroll
        for (int j = 0; j < L - 1; ++j) {
            const float* src = a.params + kH * 8 + j * (kH * kH + kH);
#pragma unroll
            for (int k = 0; k < 16; ++k) wcv[j][k] = src[tid + 256 * k];  // kH * kH = 4096
            bcv[j] = src[kH * kH + (tid & (kH - 1))];
        }
        float wov = a.params[kTail + (tid & (kH - 1))], bov = a.params[kTail + kH];
        asm volatile("" : "+v"(wov), "+v"(bov));  // keeps these two loads in the batch (hipcc sinks them below the stores)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = tid + 256 * k;
            sW1[(i >> 3) * kLdW1 + (i & 7)] = w1v[k];
        }
#pragma unroll
        for (int j = 0; j < L - 1; ++j) {
            float* dst = sWc + j * kConn;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int i = tid + 256 * k;
                dst[(i >> 6) * kLdW2 + (i & 63)] = wcv[j][k] * a.inv_keep;
            }
            if (tid < kH) dst[kH * kLdW2 + tid] = bcv[j];
        }
        if (tid < kH) sWo[tid] = wov * a.inv_keep;
        if (tid == 0) sBo[0] = bov;
    }
    __syncthreads();

    v16f gW[L - 1][2][2];
    v4f gW1[4];  // 16x16 tiles: units 16*mt4 + 4*(lane/16) + r, input column lane%16 (< 8 exist)
    float gb[L - 1][2], gwo[2] = {0.0f, 0.0f}, gbo = 0.0f, loss = 0.0f;
#pragma unroll
    for (int j = 0; j < L - 1; ++j) {
        gb[j][0] = gb[j][1] = 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) gW[j][i][0][r] = gW[j][i][1][r] = 0.0f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) gW1[i] = v4f{0.0f, 0.0f, 0.0f, 0.0f};

    // L == 2 (config 5's net): the one 64 x 64 connection also lives in REGISTERS, in the two operand layouts the
    // tile loop consumes -- forward A operand W[unit c / 32 + c][k-step's unit] and its transpose for dH -- 128 of
    // the 148 registers this instantiation leaves free (one wave per SIMD: 512 are there).  That removes 128 of a
    // tile's ~200 LDS operand reads and the waits in front of the MFMAs that consume them.  (L == 3 has no room.)
    constexpr bool kRegW = (L == 2);
    float wfw[kRegW ? 2 : 1][kRegW ? 2 : 1][kRegW ? 16 : 1], wbw[kRegW ? 2 : 1][kRegW ? 2 : 1][kRegW ? 16 : 1];
    if constexpr (kRegW) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int k = unit_of(kt, s, h);
                wfw[0][kt][s] = sWc[(c)*kLdW2 + k];
                wfw[1][kt][s] = sWc[(32 + c) * kLdW2 + k];
                wbw[0][kt][s] = sWc[k * kLdW2 + c];
                wbw[1][kt][s] = sWc[k * kLdW2 + 32 + c];
            }
    }

    for (int tile = blockIdx.x * 4 + wave; tile < a.ntiles; tile += nwaves) {
        const int64_t row = (int64_t)tile * 32 + c;
        const uint32_t drow = (a.drop_pos && a.keep16 < 65536u && row < a.nrows) ? a.drop_pos[row] : (uint32_t)row;
        const bool live = row < a.nrows;
        float4 x = xnext;
        float y = x.w;                 // upper half-wave: column 7 is the target ...
        if (h == 1) x.w = 1.0f;        // ... and its slot carries the bias input
        y = __shfl(y, c + 32, 64);
        wave_sync_lds();               // the previous tile's staging reads are done
        tX[st_idx(4 * h + 0, c)] = x.x;
        tX[st_idx(4 * h + 1, c)] = x.y;
        tX[st_idx(4 * h + 2, c)] = x.z;
        tX[st_idx(4 * h + 3, c)] = x.w;

        // ---- layer 0: Z^T [64 x 32] = W1a [64 x 8] * Xa^T [8 x 32]; k-step s <-> inputs s, s+4
        v16f act[L][2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) act[0][mt][r] = 0.0f;
            const float* wr = sW1 + (32 * mt + c) * kLdW1 + 4 * h;
            act[0][mt] = mfma(wr[0], x.x, act[0][mt]);
            act[0][mt] = mfma(wr[1], x.y, act[0][mt]);
            act[0][mt] = mfma(wr[2], x.z, act[0][mt]);
            act[0][mt] = mfma(wr[3], x.w, act[0][mt]);
        }
        // next tile's rows: issued once this tile's are consumed (a wait on the older load would
        // otherwise drain this one too), in flight for the rest of the tile
        xnext = fetch(tile + nwaves);
        relu_dropout<false>(act[0], drow, a.step, 0x100u + (uint32_t)h, a.keep16, a.inv_keep, a.k0, a.k1);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) patch[unit_base(mt, r) + so.wr[wr_sel(r)]] = act[0][mt][r];

        // ---- layers 1 .. L-1: Z_j^T = Ws_j * H_{j-1}^T + b_j; k-step (kt, s) <-> unit_of(kt, s, h)
#pragma unroll
        for (int j = 1; j < L; ++j) {
            const float* W = sWc + (j - 1) * kConn;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) act[j][mt][r] = W[kH * kLdW2 + unit_of(mt, r, h)];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const int k = unit_of(kt, s, h);
                    if constexpr (kRegW) {
                        act[j][0] = mfma(wfw[0][kt][s], act[j - 1][kt][s], act[j][0]);
                        act[j][1] = mfma(wfw[1][kt][s], act[j - 1][kt][s], act[j][1]);
                    } else {
                        act[j][0] = mfma(W[(c)*kLdW2 + k], act[j - 1][kt][s], act[j][0]);
                        act[j][1] = mfma(W[(32 + c) * kLdW2 + k], act[j - 1][kt][s], act[j][1]);
                    }
                }
            }
            relu_dropout<false>(act[j], drow, a.step, 0x100u * (uint32_t)(j + 1) + (uint32_t)h, a.keep16,
                                a.inv_keep, a.k0, a.k1);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    patch[j * kH * 32 + unit_base(mt, r) + so.wr[wr_sel(r)]] = act[j][mt][r];
        }

        // ---- output, loss, d(loss)/d(out)
        float o = 0.0f;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o = __builtin_fmaf(sWo[unit_of(mt, r, h)], act[L - 1][mt][r], o);
        o += __shfl_xor(o, 32, 64);
        o += sBo[0];
        const float diff = live ? o - y : 0.0f;
        const float dout = diff * a.two_over_b;
        if (h == 0) {
            loss = __builtin_fmaf(diff, diff, loss);
            gbo += dout;
            tX[8 * 32 + c] = dout;
        }
        // ---- back through the last activation: dz = dZ_{L-1}, B operand of the first dH product
        v16f dz[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                dz[mt][r] = act[L - 1][mt][r] > 0.0f ? sWo[unit_of(mt, r, h)] * dout : 0.0f;
        wave_sync_lds();

#pragma unroll
        for (int j = L - 1; j >= 1; --j) {
            const float* W = sWc + (j - 1) * kConn;
            const float* pA = patch + j * kH * 32;        // H_j (j = L-1: dZ_j is rebuilt from it) or dZ_j
            const float* pB = patch + (j - 1) * kH * 32;  // H_{j-1}
            // ---- gW_j [i][k] += sum_rows dZ_j[i][row] * H_{j-1}[k][row]; k-step <-> rows 16h + 4q + jj.
            // This lane owns units c and 32 + c here.  For the last hidden layer dZ of those units is
            // rebuilt from H (dZ = [H > 0] wo dout) and the output-weight gradient sum_rows dout * H
            // comes along; bias gradients are the row sums of dZ.
            const float wo0 = sWo[c], wo1 = sWo[32 + c];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 e0 = *reinterpret_cast<const float4*>(pA + so.rd[q]);
                const float4 e1 = *reinterpret_cast<const float4*>(pA + 32 * 32 + so.rd[q]);
                const float4 dq = *reinterpret_cast<const float4*>(tX + 8 * 32 + 16 * h + 4 * q);
                const float4 b0 = *reinterpret_cast<const float4*>(pB + so.rd[q]);
                const float4 b1 = *reinterpret_cast<const float4*>(pB + 32 * 32 + so.rd[q]);
                const float ev0[4] = {e0.x, e0.y, e0.z, e0.w}, ev1[4] = {e1.x, e1.y, e1.z, e1.w};
                const float dv[4] = {dq.x, dq.y, dq.z, dq.w};
                const float bv0[4] = {b0.x, b0.y, b0.z, b0.w}, bv1[4] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    float av0 = ev0[jj], av1 = ev1[jj];
                    if (j == L - 1) {
                        gwo[0] = __builtin_fmaf(dv[jj], ev0[jj], gwo[0]);
                        gwo[1] = __builtin_fmaf(dv[jj], ev1[jj], gwo[1]);
                        av0 = ev0[jj] > 0.0f ? wo0 * dv[jj] : 0.0f;
                        av1 = ev1[jj] > 0.0f ? wo1 * dv[jj] : 0.0f;
                    }
                    gb[j - 1][0] += av0;
                    gb[j - 1][1] += av1;
                    gW[j - 1][0][0] = mfma(av0, bv0[jj], gW[j - 1][0][0]);
                    gW[j - 1][0][1] = mfma(av0, bv1[jj], gW[j - 1][0][1]);
                    gW[j - 1][1][0] = mfma(av1, bv0[jj], gW[j - 1][1][0]);
                    gW[j - 1][1][1] = mfma(av1, bv1[jj], gW[j - 1][1][1]);
                }
            }
            // ---- dH_{j-1}^T = Ws_j^T * dZ_j^T, then through layer j-1's activation
            v16f d[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) d[mt][r] = 0.0f;
#pragma unroll
            for (int it = 0; it < 2; ++it) {
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    if constexpr (kRegW) {
                        d[0] = mfma(wbw[0][it][s], dz[it][s], d[0]);
                        d[1] = mfma(wbw[1][it][s], dz[it][s], d[1]);
                    } else {
                        const float* wr = W + unit_of(it, s, h) * kLdW2 + c;
                        d[0] = mfma(wr[0], dz[it][s], d[0]);
                        d[1] = mfma(wr[32], dz[it][s], d[1]);
                    }
                }
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) dz[mt][r] = act[j - 1][mt][r] > 0.0f ? d[mt][r] : 0.0f;
            wave_sync_lds();  // the product above has read patch j-1 (H_{j-1})
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    patch[(j - 1) * kH * 32 + unit_base(mt, r) + so.wr[wr_sel(r)]] = dz[mt][r];
            wave_sync_lds();
        }

        // ---- gW1a [i][n] += sum_rows dZ_0[i][row] * Xa[n][row]; only input columns n < 8 exist, so
        // this product runs on 16x16x4 tiles (unit = lane%16 + 16*mt4, column = lane%16); k-slot
        // kq = lane/16 of step s stands for row 8*kq + s: a lane reads its 8 rows as two quads
        {
            const int l16 = lane & 15, kq = lane >> 4, sw = ((l16 >> 1) & 7) << 2;
            const int o0 = l16 * 32 + ((8 * kq) ^ sw), o1 = l16 * 32 + ((8 * kq + 4) ^ sw);
            float4 bq0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), bq1 = bq0;
            if (l16 < 8) {
                bq0 = *reinterpret_cast<const float4*>(tX + o0);
                bq1 = *reinterpret_cast<const float4*>(tX + o1);
            }
            const float bv[8] = {bq0.x, bq0.y, bq0.z, bq0.w, bq1.x, bq1.y, bq1.z, bq1.w};
            float av[4][8];
#pragma unroll
            for (int mt4 = 0; mt4 < 4; ++mt4) {
                const float4 aq0 = *reinterpret_cast<const float4*>(patch + 16 * 32 * mt4 + o0);
                const float4 aq1 = *reinterpret_cast<const float4*>(patch + 16 * 32 * mt4 + o1);
                av[mt4][0] = aq0.x; av[mt4][1] = aq0.y; av[mt4][2] = aq0.z; av[mt4][3] = aq0.w;
                av[mt4][4] = aq1.x; av[mt4][5] = aq1.y; av[mt4][6] = aq1.z; av[mt4][7] = aq1.w;
            }
#pragma unroll
            for (int s8 = 0; s8 < 8; ++s8)  // the four tiles take turns: no MFMA waits for the one before it
#pragma unroll
                for (int mt4 = 0; mt4 < 4; ++mt4)
                    gW1[mt4] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt4][s8], bv[s8], gW1[mt4], 0, 0, 0);
        }
    }

    // ---- per-lane partials -> per-wave sums (a lane holds the rows of its half-wave only)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        gwo[mt] += __shfl_xor(gwo[mt], 32, 64);
#pragma unroll
        for (int j = 0; j < L - 1; ++j) gb[j][mt] += __shfl_xor(gb[j][mt], 32, 64);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        gbo += __shfl_xor(gbo, m, 64);
        loss += __shfl_xor(loss, m, 64);
    }

    // ---- the whole LDS allocation (weights are no longer needed) is re-cut into one gradient
    // vector per wave: plain stores, nothing to wait for; then the workgroup adds the copies in
    // wave order on the way out
    constexpr int GS = g_stride(L), NP = train_params(L);
    __syncthreads();
    float* G = lds + wave * GS;
#pragma unroll
    for (int j = 0; j < L - 1; ++j) {
        float* Gj = G + kH * 8 + j * (kH * kH + kH);
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = unit_of(mi, r, h);
                Gj[i * kH + c] = gW[j][mi][0][r] * a.inv_keep;
                Gj[i * kH + 32 + c] = gW[j][mi][1][r] * a.inv_keep;
            }
            if (h == 0) Gj[kH * kH + 32 * mi + c] = gb[j][mi];
        }
    }
    if (h == 0) {
        G[NP - 1 - kH + c] = gwo[0] * a.inv_keep;
        G[NP - 1 - kH + 32 + c] = gwo[1] * a.inv_keep;
    }
    if ((lane & 15) < 8) {
#pragma unroll
        for (int mt4 = 0; mt4 < 4; ++mt4)
#pragma unroll
            for (int r = 0; r < 4; ++r) G[(16 * mt4 + 4 * (lane >> 4) + r) * 8 + (lane & 15)] = gW1[mt4][r];
    }
    if (lane == 0) {
        G[NP - 1] = gbo;
        G[NP] = loss;
    }
    __syncthreads();
    float* out = a.partial + (size_t)blockIdx.x * GS;
    for (int i = tid; i <= NP; i += 256) out[i] = ((lds[i] + lds[GS + i]) + lds[2 * GS + i]) + lds[3 * GS + i];
}

__global__ __launch_bounds__(256) void mlp_adam_kernel(MlpAdamArgs a)
{
    mlp_adam_body(a);
}

// Sharded training.  (1) this rank's gradient sums of the step, partials added in mlp_adam_body's order, as doubles
// (the loss sum rides in slot nparams) -> (2) the host enqueues the all-reduce over the ranks -> (3) Adam from the
// reduced sums: mlp_adam_body with ONE partial, the float of the global sum.
__global__ __launch_bounds__(256) void mlp_grad_reduce_kernel(const float* __restrict__ partial, int nparts, int stride,
                                                              int nparams, double* __restrict__ out)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p > nparams) return;
    float g = 0.0f;
#pragma unroll 1
    for (int s0 = 0; s0 < 16; ++s0) {
        float gs = 0.0f;
        for (int w = s0; w < nparts; w += 16) gs += partial[(size_t)w * stride + p];
        g += gs;
    }
    out[p] = (double)g;
}

__global__ __launch_bounds__(256) void mlp_grad_to_float_kernel(const double* __restrict__ in, int n, float* __restrict__ out)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < n) out[p] = (float)in[p];
}

// ------------------------------------------------------------------ tile-per-wave trainer
// The same training step for the shapes and batch sizes the workgroup kernel above does not fit:
// 128 hidden units (two 128 x 128 matrices do not fit LDS beside the staging patches) and small
// minibatches (the reference's own batch of 256 rows is 8 tiles).  One wave = one 32-row tile =
// one workgroup; the A operands (weights) come straight from global memory / L2 -- tiles are few,
// so that traffic is small -- and because a wave sees exactly one tile there is nothing to
// accumulate across tiles: each 32 x H strip of a weight gradient is complete after its 16 k-steps
// and goes directly to the tile's gradient partial in global memory.
//
// Units are dealt to the 32-unit MFMA tiles round-robin: slot 32*mt + rho <-> unit NT*rho + mt
// (NT = H / 32).  A lane that owns tile-row rho = c then needs, for one k, the NT consecutive
// weights W[k][NT*c .. NT*c + NT-1]: one 16-byte load feeds NT MFMAs, and the NT accumulators of a
// gradient strip store as one 16-byte chunk per register.  LDS staging is addressed by slot (same
// patches and swizzle as above), global parameters and gradients by unit.  Forward products read a
// TRANSPOSED copy of each connection (kept up to date by the Adam kernel) so that those loads are
// row-contiguous too.
template <int NT>
struct VecN;
template <>
struct VecN<2> { typedef float2 type; };
template <>
struct VecN<4> { typedef float4 type; };
template <int NT>
__device__ __forceinline__ void load_vec(const float* p, float (&v)[NT])
{
    const typename VecN<NT>::type x = *reinterpret_cast<const typename VecN<NT>::type*>(p);
    v[0] = x.x; v[1] = x.y;
    if constexpr (NT == 4) { v[2] = x.z; v[3] = x.w; }
}
template <int NT>
__device__ __forceinline__ void store_vec(float* p, const float (&v)[NT])
{
    typename VecN<NT>::type x;
    x.x = v[0]; x.y = v[1];
    if constexpr (NT == 4) { x.z = v[2]; x.w = v[3]; }
    *reinterpret_cast<typename VecN<NT>::type*>(p) = x;
}

// concurrent waves (= gradient partials) of the tile-per-wave trainer: what fits the chip at once
__host__ __device__ constexpr int tile_waves_max(int H) { return H == 128 ? 768 : 1024; }
__host__ __device__ constexpr int tile_lds_floats(int H, int L) { return L * H * 32 + 9 * 32 + (L - 1) * H + H + 4; }

template <int H, int L>
__global__ __launch_bounds__(64) void mlp_train_tile_kernel(MlpStepArgs a, int tile0, int accumulate)
{
    constexpr int NT = H / 32, NP = mlp_params_of(H, L), CONN = H * H + H;
    constexpr int kPF = 4;  // k-steps per prefetch group
    extern __shared__ float lds[];
    float* patch = lds;                    // [L][H slots][32 rows]
    float* tX = patch + L * H * 32;        // [8][32] inputs + [32] d(loss)/d(out)
    float* sB = tX + 9 * 32;               // (L-1) x [H] biases, by slot
    float* sWo = sB + (L - 1) * H;         // output weights, by slot
    const int lane = threadIdx.x, c = lane & 31, h = lane >> 5;
    auto rho = [&](int r) { return (r >> 2) * 8 + 4 * h + (r & 3); };  // tile row of accumulator register r
    const float* Wo = a.params + H * 8 + (L - 1) * CONN;
    for (int sl = lane; sl < H; sl += 64) {
        const int unit = NT * (sl & 31) + (sl >> 5);
#pragma unroll
        for (int j = 0; j < L - 1; ++j) sB[j * H + sl] = a.params[H * 8 + j * CONN + H * H + unit];
        sWo[sl] = Wo[unit];
    }
    const StageOfs so = stage_offsets(c, h);
    float* out = a.partial + (size_t)blockIdx.x * a.pstride;
    // A minibatch of more tiles than fit the chip at once is covered by several launches of this
    // kernel: launch n handles tiles tile0 + blockIdx.x and, from the second launch on
    // (`accumulate`), adds its gradients onto the wave's partial in global memory -- accumulators
    // start from the stored strip instead of zero.
    const int tile = tile0 + blockIdx.x;
    if (tile >= a.ntiles) return;
    const bool first = !accumulate;
    const int64_t row = (int64_t)tile * 32 + c;
    const uint32_t drow = (a.drop_pos && a.keep16 < 65536u && row < a.nrows) ? a.drop_pos[row] : (uint32_t)row;
    const bool live = row < a.nrows;
    float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live) x = reinterpret_cast<const float4*>(a.data + shuffle_index(a.shuf, (uint64_t)(a.row0 + row)) * 8)[h];
    float y = x.w;
    if (h == 1) x.w = 1.0f;
    y = __shfl(y, c + 32, 64);
    tX[st_idx(4 * h + 0, c)] = x.x;
    tX[st_idx(4 * h + 1, c)] = x.y;
    tX[st_idx(4 * h + 2, c)] = x.z;
    tX[st_idx(4 * h + 3, c)] = x.w;

    // ---- layer 0
    v16f act[L][NT];
#pragma unroll
    for (int mt = 0; mt < NT; ++mt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) act[0][mt][r] = 0.0f;
        const float4 w = *reinterpret_cast<const float4*>(a.params + (NT * c + mt) * 8 + 4 * h);
        act[0][mt] = mfma(w.x, x.x, act[0][mt]);
        act[0][mt] = mfma(w.y, x.y, act[0][mt]);
        act[0][mt] = mfma(w.z, x.z, act[0][mt]);
        act[0][mt] = mfma(w.w, x.w, act[0][mt]);
    }
    relu_dropout_t<NT, true>(act[0], drow, a.step, 0x100u + (uint32_t)h, a.keep16, a.inv_keep, a.k0, a.k1);
#pragma unroll
    for (int mt = 0; mt < NT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) patch[unit_base(mt, r) + so.wr[wr_sel(r)]] = act[0][mt][r];
    wave_sync_lds();  // biases, inputs

    // ---- layers 1 .. L-1: A = Wt_j[k][NT*c ..], one vector load per k-step feeds the NT tiles
#pragma unroll
    for (int j = 1; j < L; ++j) {
        const float* Wt = a.wt + (size_t)(j - 1) * H * H;
#pragma unroll
        for (int mt = 0; mt < NT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) act[j][mt][r] = sB[(j - 1) * H + 32 * mt + rho(r)];
        // weights of the next group of kPF k-steps are requested before the current group's MFMAs
        // are issued: an L2 round trip is several MFMA groups long
        {
            float w[2][kPF][NT];
            auto fetch_group = [&](int g, float (&dst)[kPF][NT]) {
#pragma unroll
                for (int i = 0; i < kPF; ++i) {
                    const int ks = g * kPF + i, kt = ks >> 4, s = ks & 15;
                    load_vec<NT>(Wt + (size_t)(NT * rho(s) + kt) * H + NT * c, dst[i]);
                }
            };
            fetch_group(0, w[0]);
#pragma unroll
            for (int g = 0; g < NT * 16 / kPF; ++g) {
                if (g + 1 < NT * 16 / kPF) fetch_group(g + 1, w[(g + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < kPF; ++i) {
                    const int ks = g * kPF + i, kt = ks >> 4, s = ks & 15;
#pragma unroll
                    for (int mt = 0; mt < NT; ++mt)
                        act[j][mt] = mfma(w[g & 1][i][mt], act[j - 1][kt][s], act[j][mt]);
                }
            }
        }
        relu_dropout_t<NT, true>(act[j], drow, a.step, 0x100u * (uint32_t)(j + 1) + (uint32_t)h, a.keep16,
                                 a.inv_keep, a.k0, a.k1);
#pragma unroll
        for (int mt = 0; mt < NT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) patch[j * H * 32 + unit_base(mt, r) + so.wr[wr_sel(r)]] = act[j][mt][r];
    }

    // ---- output, loss, d(loss)/d(out)
    float o = 0.0f;
#pragma unroll
    for (int mt = 0; mt < NT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o = __builtin_fmaf(sWo[32 * mt + rho(r)], act[L - 1][mt][r], o);
    o += __shfl_xor(o, 32, 64);
    o += Wo[H];
    const float diff = live ? o - y : 0.0f;
    const float dout = diff * a.two_over_b;
    if (h == 0) tX[8 * 32 + c] = dout;
    v16f dz[NT];
#pragma unroll
    for (int mt = 0; mt < NT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            dz[mt][r] = act[L - 1][mt][r] > 0.0f ? sWo[32 * mt + rho(r)] * dout * a.inv_keep : 0.0f;
    wave_sync_lds();

#pragma unroll
    for (int j = L - 1; j >= 1; --j) {
        const float* W = a.params + H * 8 + (size_t)(j - 1) * CONN;
        float* gWj = out + H * 8 + (size_t)(j - 1) * CONN;
        const float* pA = patch + j * H * 32;
        const float* pB = patch + (j - 1) * H * 32;
        // ---- gW_j strip by strip: rows i = slots 32*mi + c, all H columns; complete after 16 k-steps
#pragma unroll
        for (int mi = 0; mi < NT; ++mi) {
            v16f acc[NT];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v[NT];
#pragma unroll
                for (int ni = 0; ni < NT; ++ni) v[ni] = 0.0f;
                if (!first) load_vec<NT>(gWj + (size_t)(NT * rho(r) + mi) * H + NT * c, v);
#pragma unroll
                for (int ni = 0; ni < NT; ++ni) acc[ni][r] = v[ni];
            }
            const float woi = sWo[32 * mi + c] * a.inv_keep;
            float gbs = 0.0f, gws = 0.0f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 e = *reinterpret_cast<const float4*>(pA + 32 * 32 * mi + so.rd[q]);
                const float4 dq = *reinterpret_cast<const float4*>(tX + 8 * 32 + 16 * h + 4 * q);
                const float ev[4] = {e.x, e.y, e.z, e.w}, dv[4] = {dq.x, dq.y, dq.z, dq.w};
                float bv[NT][4];
#pragma unroll
                for (int ni = 0; ni < NT; ++ni) {
                    const float4 b = *reinterpret_cast<const float4*>(pB + 32 * 32 * ni + so.rd[q]);
                    bv[ni][0] = b.x; bv[ni][1] = b.y; bv[ni][2] = b.z; bv[ni][3] = b.w;
                }
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    float av = ev[jj];
                    if (j == L - 1) {
                        gws = __builtin_fmaf(dv[jj], ev[jj], gws);
                        av = ev[jj] > 0.0f ? woi * dv[jj] : 0.0f;
                    }
                    gbs += av;
#pragma unroll
                    for (int ni = 0; ni < NT; ++ni) acc[ni] = mfma(av, bv[ni][jj], acc[ni]);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v[NT];
#pragma unroll
                for (int ni = 0; ni < NT; ++ni) v[ni] = acc[ni][r];
                store_vec<NT>(gWj + (size_t)(NT * rho(r) + mi) * H + NT * c, v);
            }
            gbs += __shfl_xor(gbs, 32, 64);
            gws += __shfl_xor(gws, 32, 64);
            if (h == 0) {
                float* pb = gWj + H * H + NT * c + mi;
                *pb = first ? gbs : *pb + gbs;
                if (j == L - 1) {
                    float* pw = out + H * 8 + (L - 1) * CONN + NT * c + mi;
                    *pw = first ? gws : *pw + gws;
                }
            }
        }
        // ---- dH_{j-1} = W_j^T dZ_j: A = W_j[i][NT*c ..]
        v16f d[NT];
#pragma unroll
        for (int mt = 0; mt < NT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) d[mt][r] = 0.0f;
        {
            float w[2][kPF][NT];
            auto fetch_group = [&](int g, float (&dst)[kPF][NT]) {
#pragma unroll
                for (int i = 0; i < kPF; ++i) {
                    const int ks = g * kPF + i, it = ks >> 4, s = ks & 15;
                    load_vec<NT>(W + (size_t)(NT * rho(s) + it) * H + NT * c, dst[i]);
                }
            };
            fetch_group(0, w[0]);
#pragma unroll
            for (int g = 0; g < NT * 16 / kPF; ++g) {
                if (g + 1 < NT * 16 / kPF) fetch_group(g + 1, w[(g + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < kPF; ++i) {
                    const int ks = g * kPF + i, it = ks >> 4, s = ks & 15;
#pragma unroll
                    for (int mt = 0; mt < NT; ++mt) d[mt] = mfma(w[g & 1][i][mt], dz[it][s], d[mt]);
                }
            }
        }
#pragma unroll
        for (int mt = 0; mt < NT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) dz[mt][r] = act[j - 1][mt][r] > 0.0f ? d[mt][r] * a.inv_keep : 0.0f;
        wave_sync_lds();
#pragma unroll
        for (int mt = 0; mt < NT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) patch[(j - 1) * H * 32 + unit_base(mt, r) + so.wr[wr_sel(r)]] = dz[mt][r];
        wave_sync_lds();
    }

    // ---- gW1a: 16x16x4 tiles over slots 16*mt4 + lane%16, k-slot lane/16 of step s <-> row 8*kq + s
    {
        const int l16 = lane & 15, kq = lane >> 4, sw = ((l16 >> 1) & 7) << 2;
        const int o0 = l16 * 32 + ((8 * kq) ^ sw), o1 = l16 * 32 + ((8 * kq + 4) ^ sw);
        float4 bq0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), bq1 = bq0;
        if (l16 < 8) {
            bq0 = *reinterpret_cast<const float4*>(tX + o0);
            bq1 = *reinterpret_cast<const float4*>(tX + o1);
        }
        const float bv[8] = {bq0.x, bq0.y, bq0.z, bq0.w, bq1.x, bq1.y, bq1.z, bq1.w};
#pragma unroll
        for (int mt4 = 0; mt4 < H / 16; ++mt4) {
            const float4 aq0 = *reinterpret_cast<const float4*>(patch + 16 * 32 * mt4 + o0);
            const float4 aq1 = *reinterpret_cast<const float4*>(patch + 16 * 32 * mt4 + o1);
            const float av[8] = {aq0.x, aq0.y, aq0.z, aq0.w, aq1.x, aq1.y, aq1.z, aq1.w};
            v4f g = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int s8 = 0; s8 < 8; ++s8) g = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s8], bv[s8], g, 0, 0, 0);
            if (l16 < 8) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int slot = 16 * mt4 + 4 * (lane >> 4) + r;
                    float* pg = out + (NT * (slot & 31) + (slot >> 5)) * 8 + l16;
                    *pg = first ? g[r] : *pg + g[r];
                }
            }
        }
    }
    float gbo = h == 0 ? dout : 0.0f, loss = h == 0 ? diff * diff : 0.0f;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        gbo += __shfl_xor(gbo, m, 64);
        loss += __shfl_xor(loss, m, 64);
    }
    if (lane == 0) {
        out[NP - 1] = first ? gbo : out[NP - 1] + gbo;
        out[NP] = first ? loss : out[NP] + loss;
    }
}

// ------------------------------------------------------------------ tile-per-workgroup trainers (omc_mlp_quad_dev.h)
template <int H, int L>
__global__ __launch_bounds__(H * 2) void mlp_train_quad_kernel(MlpStepArgs a)
{
    mlp_train_quad_body<H, L>(a, blockIdx.x);
}

template <int H, int L>
__global__ __launch_bounds__(H * 2) void mlp_train_q16_kernel(MlpStepArgs a)
{
    mlp_train_q16_body<H, L>(a, blockIdx.x);
}

// wt_j[k][i] = W_j[i][k] for the L-1 connections (start of an epoch; Adam keeps it current)
__global__ __launch_bounds__(256) void mlp_transpose_kernel(const float* params, float* wt, int H, int L)
{
    const int n = (L - 1) * H * H;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < n; idx += gridDim.x * 256) {
        const int j = idx / (H * H), rem = idx - j * H * H, k = rem / H, i = rem - k * H;
        wt[idx] = params[H * 8 + j * (H * H + H) + i * H + k];
    }
}

}  // namespace

// Which kernel trains (hidden, layers) at this minibatch size (MlpKernel, omc_kernels.h; the numbers are ABI):
//   kGroup  64 units at more than 32 tiles of 32 rows: the workgroup kernel, weights in LDS;
//   kTile   one wave per tile: 128 units above kMlpMaxGroups tiles (and every 64 / 128-unit quad case when
//           OMC_MLP_QUAD=0 switches the tile-per-workgroup kernels off: A/B measurements);
//   kQuad   one workgroup per 32-row tile: 64 units up to 32 tiles, 128 units up to kMlpMaxGroups tiles (the
//           reference's batch of 256 rows is 8), 32 units (the per-step ContNet of omc_contnet.hip) at any size;
//   kQ16    kQuad's cases of 64 / 128 units at up to mlp_q16_rows() rows: 16-row tiles;
//   kNone   no trainer for this shape.
// `batch` is the GLOBAL minibatch size, sharded or not (mlp_plan_kernel_batch).  A rank's own part of a minibatch is
// never larger (omc_mlp_train_epoch_sharded checks step_off against it), so the partial buffer sized by it covers the
// rank; and every rank of a job -- and the unsharded run of the same job -- picks the SAME kernel, hence the same
// dropout tags and unit map: a rank's masks are those of the unsharded run whatever its share of a minibatch is (a
// choice by the local share used to split ranks at the 4,096-row limit of the 16-row kernel: ADVICE r5).
// mlp_train_kernel_choice32: the choice before the 16-row tiles existed -- what the side-by-side trainers start from.
static MlpKernel mlp_train_kernel_choice32(int hidden, int layers, int64_t batch)
{
    if (layers != 2 && layers != 3) return kNone;
    const int64_t tiles = (batch + 31) / 32;
    static const int quad = getenv("OMC_MLP_QUAD") ? atoi(getenv("OMC_MLP_QUAD")) : 1;
    if (hidden == 64) return tiles <= 32 ? (quad ? kQuad : kTile) : kGroup;
    if (hidden == 128) return (quad && tiles <= kMlpMaxGroups) ? kQuad : kTile;
    if (hidden == 32) return kQuad;
    return kNone;
}

// 16-row tiles while a minibatch does not fill the chip (kMlpQ16MaxRows rows = 256 workgroups; measured at 3 x 128: 28.4
// against 30.2 us per step at 1,024 rows, a tie at 2,048, 37.4 against 40.0 at 4,096, 57 against 45 at 8,192): the reference's
// own min(256, R).  OMC_MLP_Q16=0 switches them off, =N moves the limit to N rows (A/B measurements).
int64_t mlp_q16_rows(int hidden)
{
    static const int q16 = getenv("OMC_MLP_Q16") ? atoi(getenv("OMC_MLP_Q16")) : -1;
    if (hidden != 64 && hidden != 128) return 0;
    return q16 < 0 ? kMlpQ16MaxRows : q16;
}

MlpKernel mlp_train_kernel_choice(int hidden, int layers, int64_t batch)
{
    const MlpKernel c = mlp_train_kernel_choice32(hidden, layers, batch);
    return (c == kQuad && batch <= mlp_q16_rows(hidden)) ? kQ16 : c;
}

int64_t mlp_plan_kernel_batch(const MlpTrainPlan& t) { return t.batch; }

// the side-by-side trainers (omc_mlp_batch.hip) wrap the tile-per-workgroup bodies only
bool mlp_batch_supported(int hidden, int layers, int64_t batch)
{
    return mlp_train_kernel_choice32(hidden, layers, batch) == kQuad;
}

int mlp_param_count(int hidden, int layers)
{
    if ((hidden != 32 && hidden != 64 && hidden != 128) || (layers != 2 && layers != 3)) return -1;
    return mlp_params_of(hidden, layers);
}

size_t mlp_partial_bytes(int hidden, int layers, int64_t batch)
{
    const int64_t tiles = (batch + 31) / 32, cap = tile_waves_max(hidden);
    switch (mlp_train_kernel_choice(hidden, layers, batch)) {
    case kGroup: return sizeof(float) * (size_t)kMlpMaxGroups * kMlpPartialStride3;
    case kQ16: return sizeof(float) * (size_t)((batch + 15) / 16) * tile_pstride(hidden, layers);
    case kTile:
    case kQuad:
        // 32 units: one partial per tile however many (the kernel never accumulates across tiles)
        return sizeof(float) * (size_t)(hidden == 32 || tiles < cap ? tiles : cap) * tile_pstride(hidden, layers);
    case kNone: break;
    }
    return 0;
}

size_t mlp_wt_bytes(int hidden, int layers) { return sizeof(float) * (size_t)(layers - 1) * hidden * hidden; }

// ------------------------------------------------------------------ the optimizer steps of one epoch
// Step k trains on `local` rows starting at `row0` of t.data and is one minibatch of `global` rows (single GPU: the
// same thing; sharded: this rank's part of the job's minibatch).
struct StepSpan { int64_t row0, local, global; };
static inline int64_t plan_steps(const MlpTrainPlan& t)
{
    const int64_t rows = t.step_off ? t.rows_global : t.nrows;
    return (rows + t.batch - 1) / t.batch;
}
static inline StepSpan plan_span(const MlpTrainPlan& t, int64_t k)
{
    const int64_t rows = t.step_off ? t.rows_global : t.nrows;
    const int64_t o = k * t.batch, g = rows - o < t.batch ? rows - o : t.batch;
    if (!t.step_off) return {o, g, g};
    return {t.step_off[k], t.step_off[k + 1] - t.step_off[k], g};
}
static inline Shuffle plan_shuffle(const MlpTrainPlan& t)
{
    return t.step_off ? make_shuffle(t.nrows, 0) : make_shuffle(t.nrows, t.shuffle_key);  // sharded: rows are in epoch order
}

// After the forward / backward launch(es) of a step: Adam on this rank's partials, or -- sharded -- on the sum of all
// ranks' partials.  `b` is complete except for the partial source.  -> 0 or the all-reduce's error.
static int finish_step(hipStream_t st, const MlpTrainPlan& t, MlpAdamArgs b)
{
    const int adam_blocks = (b.nparams + 16) / 16;
    if (t.step_off) {
        const int n = b.nparams + 1;
        hipLaunchKernelGGL(mlp_grad_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, st, b.partial, b.nparts, b.stride,
                           b.nparams, t.gred);
        const int rc = t.allreduce(t.allreduce_user, t.gred, n);
        if (rc) return rc;
        float* gf = reinterpret_cast<float*>(t.gred + n);  // [n] floats behind the doubles
        hipLaunchKernelGGL(mlp_grad_to_float_kernel, dim3((n + 255) / 256), dim3(256), 0, st, t.gred, n, gf);
        b.partial = gf;
        b.nparts = 1;
        b.stride = n;
    }
    hipLaunchKernelGGL(mlp_adam_kernel, dim3(adam_blocks), dim3(256), 0, st, b);
    return 0;
}

// What the step loop has to know about a trainer; `launch(a)` enqueues the step's forward / backward kernel(s) and
// returns how many partials they write.
struct Trainer {
    int H, L;
    int tile_rows;  // rows of a tile
    int pstride;    // floats between gradient partials
    bool uses_wt;   // reads the transposed connections: made at entry unless current, kept so by Adam
};

template <class Launch>
static hipError_t run_steps(hipStream_t st, const MlpTrainPlan& t, const Trainer& tr, Launch&& launch)
{
    if (tr.uses_wt && !t.wt_current)
        hipLaunchKernelGGL(mlp_transpose_kernel, dim3(64), dim3(256), 0, st, t.params, t.wt, tr.H, tr.L);
    const MlpNet net = mlp_net(t.data, t.params, t.adam_m, t.adam_v, t.partial, tr.uses_wt ? t.wt : nullptr, t.loss_acc, t.lr,
                               t.beta1, t.beta2, t.eps, t.weight_decay, plan_shuffle(t), t.dropout, t.seed, tr.pstride);
    int64_t step = t.first_step;
    const int64_t nsteps = plan_steps(t);
    for (int64_t k = 0; k < nsteps; ++k) {
        const StepSpan sp = plan_span(t, k);
        ++step;
        MlpStepArgs a = mlp_step_args(net, sp.row0, sp.local, sp.global, tr.tile_rows, step);
        a.drop_pos = t.drop_pos ? t.drop_pos + sp.row0 : nullptr;
        const int nparts = launch(a);  // (a rank may own no row of a step: nothing is launched, Adam sums 0 partials)
        const double bc1 = 1.0 - pow(t.beta1, (double)step), bc2 = 1.0 - pow(t.beta2, (double)step);
        if (finish_step(st, t, mlp_adam_args(net, nparts, tr.H, tr.L, sp.global, bc1, bc2))) return hipErrorUnknown;
    }
    return hipGetLastError();
}

template <int L>
static hipError_t group_steps(hipStream_t st, const MlpTrainPlan& t)
{
    static std::atomic<uint64_t> attr_mask{0};  // per device (omc_kernels.h)
    const size_t lds_bytes = sizeof(float) * (size_t)train_lds_floats(L);
    hipError_t e = set_max_dynamic_lds(attr_mask, reinterpret_cast<const void*>(mlp_train_kernel<L>), lds_bytes);
    if (e != hipSuccess) return e;
    return run_steps(st, t, Trainer{kH, L, 32, g_stride(L), false}, [&](const MlpStepArgs& a) {
        const int groups = std::min((a.ntiles + 3) / 4, kMlpMaxGroups);
        if (groups > 0) hipLaunchKernelGGL(mlp_train_kernel<L>, dim3(groups), dim3(256), lds_bytes, st, a);
        return groups;
    });
}

template <int H, int L>
static hipError_t tile_steps(hipStream_t st, const MlpTrainPlan& t)
{
    static std::atomic<uint64_t> attr_mask{0};  // per device (omc_kernels.h)
    const size_t lds_bytes = sizeof(float) * (size_t)tile_lds_floats(H, L);
    if (lds_bytes > 48 * 1024) {
        hipError_t e = set_max_dynamic_lds(attr_mask, reinterpret_cast<const void*>(mlp_train_tile_kernel<H, L>), lds_bytes);
        if (e != hipSuccess) return e;
    }
    return run_steps(st, t, Trainer{H, L, 32, tile_pstride(H, L), true}, [&](const MlpStepArgs& a) {
        // more tiles than fit the chip at once: several launches, the later ones add onto the waves' partials
        const int waves = std::min(a.ntiles, tile_waves_max(H));
        for (int t0 = 0; t0 < a.ntiles; t0 += waves)
            hipLaunchKernelGGL((mlp_train_tile_kernel<H, L>), dim3(waves), dim3(64), lds_bytes, st, a, t0, (int)(t0 > 0));
        return waves;
    });
}

// one workgroup per tile, one partial each (mlp_train_quad_kernel: 32-row tiles; mlp_train_q16_kernel: 16-row tiles)
template <int H, int L, bool Q16>
static hipError_t quad_steps(hipStream_t st, const MlpTrainPlan& t)
{
    return run_steps(st, t, Trainer{H, L, Q16 ? 16 : 32, tile_pstride(H, L), true}, [&](const MlpStepArgs& a) {
        if (a.ntiles > 0) {
            if constexpr (Q16) hipLaunchKernelGGL((mlp_train_q16_kernel<H, L>), dim3(a.ntiles), dim3(H * 2), 0, st, a);
            else hipLaunchKernelGGL((mlp_train_quad_kernel<H, L>), dim3(a.ntiles), dim3(H * 2), 0, st, a);
        }
        return a.ntiles;
    });
}

hipError_t mlp_train_steps(hipStream_t st, const MlpTrainPlan& t)
{
    MlpKernel choice = mlp_train_kernel_choice(t.hidden, t.layers, mlp_plan_kernel_batch(t));
    if (choice == kQ16 && !t.allow_q16) choice = kQuad;  // (kQ16 is only ever returned where kQuad applies)
    // built for: kGroup 64 units; kTile and kQ16 64 / 128 units; kQuad 32 / 64 / 128 units; 2 / 3 layers each
    return dispatch_hl(t.hidden, t.layers, [&](auto h, auto l) -> hipError_t {
        constexpr int H = decltype(h)::value, L = decltype(l)::value;
        if (choice == kQuad) return quad_steps<H, L, false>(st, t);
        if constexpr (H >= 64) {
            if (choice == kQ16) return quad_steps<H, L, true>(st, t);
            if (choice == kTile) return tile_steps<H, L>(st, t);
        }
        if constexpr (H == kH) {
            if (choice == kGroup) return group_steps<L>(st, t);
        }
        return hipErrorInvalidValue;
    });
}

}  // namespace omc
