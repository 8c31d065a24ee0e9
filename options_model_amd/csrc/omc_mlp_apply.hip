// omc_mlp_apply.hip -- networks evaluated inside a sweep over the time steps, no training.  In this file:
//   * mlp_apply_kernel / mlp_apply_pass2: pass 2 of the NN flow, the sticky backward sweep with the trained
//     continuation-value network (32 / 64 / 128 units x 2 / 3 hidden layers) deciding exercise, dropout active when asked;
//   * localvol_paths_kernel / localvol_paths: local-vol path simulation through the implied-vol network (row f-4; a
//     different network: 2 inputs, GELU, LayerNorm, residual blocks);
//   * mlp_mask_probe_kernel / mlp_dropout_masks: which units the dropout of pass 2 and of each trainer keeps -- the
//     device half of the known-answer test against oracle/dropout.py.
// Both sweeps keep activations in the trainers' transposed MFMA accumulator layout (omc_mlp_dev.h).
#include "omc_mlp_dev.h"

namespace omc {

namespace {

// ------------------------------------------------------------------ pass 2 with the network
// Sticky backward sweep of the NN flow (options_model_3.py:615-649): at every step the
// continuation value of every still-alive in-the-money path is the network's output on the
// normalised features; exercise where payoff > continuation (strict), first hit going backwards
// sticks.  One wave owns 32 paths for the whole sweep (state in registers), the forward pass
// is the training kernel's (float32 MFMA, transposed layout), dropout stays ACTIVE when asked
// for (the reference never switches the net to eval mode).  Leaves (sx, tex)
// for the common valuation kernel.
struct MlpApplyArgs {
    const float* S;
    int64_t ld, M;
    int N, is_put;
    double K, T, dt;
    const float* params;
    double fm[7], rs[7];  // feature means, reciprocal stds
    double ym, ysd;
    float* sx;
    int32_t* tex;
    float inv_keep;
    uint32_t keep16, k0, k1;
    int ntiles;
    // dropout key of column p: its column in the UNSHARDED matrix (p + base0 for the first half of this matrix's
    // columns, p - half + base1 for the second), so that a shard draws the masks the single GPU draws
    int64_t key_half, key_base0, key_base1;
};

__host__ __device__ constexpr int apply_lds_floats(int H, int L)
{
    return H * kLdW1 + (L - 1) * (H * (H + 1) + H) + H + 4;
}

template <int H, int L>
__global__ __launch_bounds__(256) void mlp_apply_kernel(MlpApplyArgs a)
{
    constexpr int NT = H / 32, LDW = H + 1;
    extern __shared__ float sw[];
    float* sW1 = sw;                       // [H][9]
    float* sWh = sW1 + H * kLdW1;          // (L-1) x { [H][H+1], bias [H] }
    float* sWo = sWh + (L - 1) * (H * LDW + H);
    float* sBo = sWo + H;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, h = lane >> 5;
    // (stage_block: a chunk's loads are all in flight before its first LDS store, omc_device.h)
    stage_block(a.params, H * 8, tid, [&](int i, float v) { sW1[(i >> 3) * kLdW1 + (i & 7)] = v; });
#pragma unroll
    for (int l = 0; l < L - 1; ++l) {
        const float* src = a.params + H * 8 + l * (H * H + H);
        float* dst = sWh + l * (H * LDW + H);
        stage_block(src, H * H + H, tid, [&](int i, float v) {  // weights [H][H] -> [H][H + 1], then the bias row
            if (i < H * H) dst[(i / H) * LDW + (i % H)] = v;
            else dst[H * LDW + (i - H * H)] = v;
        });
    }
    stage_block(a.params + H * 8 + (L - 1) * (H * H + H), H + 1, tid, [&](int i, float v) {
        if (i < H) sWo[i] = v;
        else sBo[0] = v;
    });
    __syncthreads();
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= a.ntiles) return;  // whole wave; no barrier below
    const int64_t p = (int64_t)tile * 32 + c;
    const bool live = p < a.M;
    const float* col = a.S + (live ? p : a.M - 1);
    const uint32_t pk = (uint32_t)(p < a.key_half ? p + a.key_base0 : p - a.key_half + a.key_base1);  // dropout key
    const double K = a.K;
    const uint32_t rtag = (uint32_t)h + 2u * (uint32_t)(p >> 32);
    float sx = col[(int64_t)a.N * a.ld];
    int tex = a.N;
    bool done = !live;
    float s_next = a.N > 1 ? col[(int64_t)(a.N - 1) * a.ld] : 0.0f;
    for (int t = a.N - 1; t >= 1; --t) {
        const float sf = s_next;
        if (t > 1) s_next = col[(int64_t)(t - 1) * a.ld];
        const double sd = (double)sf;
        const double imm = a.is_put ? K - sd : sd - K;
        const bool need = !done && imm > 0.0;
        if (__builtin_amdgcn_ballot_w64(need) == 0) continue;  // nobody to decide for (uniform)
        const double x = sd / K;
        const double st = sqrt(fmax(a.T - (double)t * a.dt, 1e-6));
        float4 xin;
        if (h == 0) {
            xin.x = (float)((1.0 - a.fm[0]) * a.rs[0]);
            xin.y = (float)((x - a.fm[1]) * a.rs[1]);
            xin.z = (float)((x * x - a.fm[2]) * a.rs[2]);
            xin.w = (float)((x * x * x - a.fm[3]) * a.rs[3]);
        } else {
            xin.x = (float)((fmax(x - 1.0, 0.0) - a.fm[4]) * a.rs[4]);
            xin.y = (float)((st - a.fm[5]) * a.rs[5]);
            xin.z = (float)((x * st - a.fm[6]) * a.rs[6]);
            xin.w = 1.0f;  // bias input
        }
        v16f act[NT];
#pragma unroll
        for (int mt = 0; mt < NT; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) act[mt][r] = 0.0f;
            const float* wr = sW1 + (32 * mt + c) * kLdW1 + 4 * h;
            act[mt] = mfma(wr[0], xin.x, act[mt]);
            act[mt] = mfma(wr[1], xin.y, act[mt]);
            act[mt] = mfma(wr[2], xin.z, act[mt]);
            act[mt] = mfma(wr[3], xin.w, act[mt]);
        }
        relu_dropout_n<NT>(act, pk, (uint32_t)t, 0x300u + rtag, a.keep16, a.inv_keep, a.k0, a.k1);
#pragma unroll
        for (int l = 0; l < L - 1; ++l) {
            const float* W = sWh + l * (H * LDW + H);
            const float* B = W + H * LDW;
            v16f nxt[NT];
#pragma unroll
            for (int mt = 0; mt < NT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) nxt[mt][r] = B[unit_of(mt, r, h)];
#pragma unroll
            for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const int k = unit_of(kt, s, h);
#pragma unroll
                    for (int mt = 0; mt < NT; ++mt) nxt[mt] = mfma(W[(32 * mt + c) * LDW + k], act[kt][s], nxt[mt]);
                }
            }
            relu_dropout_n<NT>(nxt, pk, (uint32_t)t, 0x400u + 0x100u * (uint32_t)l + rtag, a.keep16,
                               a.inv_keep, a.k0, a.k1);
#pragma unroll
            for (int mt = 0; mt < NT; ++mt) act[mt] = nxt[mt];
        }
        float o = 0.0f;
#pragma unroll
        for (int mt = 0; mt < NT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o = __builtin_fmaf(sWo[unit_of(mt, r, h)], act[mt][r], o);
        o += __shfl_xor(o, 32, 64);
        o += sBo[0];
        const double cont = (double)o * a.ysd + a.ym;
        if (need && imm > cont) {
            done = true;
            tex = t;
            sx = sf;
        }
    }
    if (live && h == 0) {
        a.sx[p] = sx;
        a.tex[p] = tex;
    }
}

// ------------------------------------------------------------------ local-vol paths (row f-4)
// simulate_local_vol_paths_antithetic (options_model_3.py:300-333) with the implied-vol network
// (ImprovedIVNetwork, NN_training_stock_iv.py:109-155: Linear(2,64)+GELU, L x [h += GELU(
// LayerNorm(Linear(h)))], Linear(64,1) clamped at epsilon; dropout is off in eval mode) evaluated
// inside the path loop: one wave carries 32 columns through all time steps, activations stay in
// the transposed MFMA accumulator layout of the trainers (lane <-> column), so LayerNorm's
// sums over the 64 units are sums over a lane's registers plus one swap between half-waves.
// Flat parameters: Win|bin as [64][4] (w_m, w_tau, bias, 0), per layer W [64][64], b, gamma,
// beta [64] each, then the output weights [64] and bias [1].
struct LocalVolArgs {
    float* S;
    int64_t ld, M, P;
    int N, L;
    const float* params;
    const float* Z;  // [N][P] normals of the first half; the partner column uses -z
    float s0, r, dt, sqdt, eps_out;
    double K, T, dtd, inv_m_scale, inv_tau_scale;
    int ntiles;
};

__device__ __forceinline__ float gelu_exact(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }

__global__ __launch_bounds__(256) void localvol_paths_kernel(LocalVolArgs a)
{
    constexpr int kLayer = kH * kLdW2 + 3 * kH;
    extern __shared__ float sw[];
    float* sWin = sw;                 // [64][4]
    float* sLay = sWin + kH * 4;      // L x { W [64][65], b, gamma, beta }
    float* sWo = sLay + a.L * kLayer;  // [64] + bias
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, h = lane >> 5;
    stage_block(a.params, kH * 4, tid, [&](int i, float v) { sWin[i] = v; });
    for (int l = 0; l < a.L; ++l) {
        const float* src = a.params + kH * 4 + l * (kH * kH + 3 * kH);
        float* dst = sLay + l * kLayer;
        stage_block(src, kH * kH + 3 * kH, tid, [&](int i, float v) {
            if (i < kH * kH) dst[(i >> 6) * kLdW2 + (i & 63)] = v;
            else dst[kH * kLdW2 + (i - kH * kH)] = v;
        });
    }
    stage_block(a.params + kH * 4 + a.L * (kH * kH + 3 * kH), kH + 1, tid, [&](int i, float v) { sWo[i] = v; });
    __syncthreads();
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= a.ntiles) return;  // whole wave; no barrier below
    const int64_t col = (int64_t)tile * 32 + c;
    const bool live = col < a.M;
    const int64_t zc = live ? (col < a.P ? col : col - a.P) : 0;
    const float zs = col < a.P ? 1.0f : -1.0f;
    float s = a.s0;
    if (live && h == 0) a.S[col] = s;
    float z_next = a.Z[zc];
    for (int t = 1; t <= a.N; ++t) {
        const float z = z_next * zs;
        if (t < a.N) z_next = a.Z[(int64_t)t * a.P + zc];
        const double tau = fmax(a.T - (double)(t - 1) * a.dtd, 1e-6);
        const float xin = h == 0 ? (float)(log(fmax(a.K, 1e-8) / fmax((double)s, 1e-8)) * a.inv_m_scale)
                                 : (float)(tau * a.inv_tau_scale);
        v16f act[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) act[mt][r] = sWin[unit_of(mt, r, h) * 4 + 2];
            act[mt] = mfma(sWin[(32 * mt + c) * 4 + h], xin, act[mt]);
#pragma unroll
            for (int r = 0; r < 16; ++r) act[mt][r] = gelu_exact(act[mt][r]);
        }
        for (int l = 0; l < a.L; ++l) {
            const float* W = sLay + l * kLayer;
            const float* B = W + kH * kLdW2;
            v16f zz[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) zz[mt][r] = B[unit_of(mt, r, h)];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
                for (int sI = 0; sI < 16; ++sI) {
                    const int k = unit_of(kt, sI, h);
                    zz[0] = mfma(W[(c)*kLdW2 + k], act[kt][sI], zz[0]);
                    zz[1] = mfma(W[(32 + c) * kLdW2 + k], act[kt][sI], zz[1]);
                }
            }
            // LayerNorm over the 64 units of a column: this lane's 32 + the other half-wave's 32
            float sum = 0.0f;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) sum += zz[mt][r];
            sum += __shfl_xor(sum, 32, 64);
            const float mean = sum * (1.0f / 64.0f);
            float sq = 0.0f;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float d = zz[mt][r] - mean;
                    sq = __builtin_fmaf(d, d, sq);
                }
            sq += __shfl_xor(sq, 32, 64);
            const float rstd = 1.0f / __builtin_sqrtf(sq * (1.0f / 64.0f) + 1e-5f);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int u = unit_of(mt, r, h);
                    const float y = (zz[mt][r] - mean) * rstd * B[kH + u] + B[2 * kH + u];
                    act[mt][r] += gelu_exact(y);
                }
        }
        float o = 0.0f;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o = __builtin_fmaf(sWo[unit_of(mt, r, h)], act[mt][r], o);
        o += __shfl_xor(o, 32, 64);
        o += sWo[kH];
        const float sig = fmaxf(fmaxf(o, a.eps_out), 1e-6f);
        s = s * expf((a.r - 0.5f * sig * sig) * a.dt + sig * a.sqdt * z);
        if (live && h == 0) a.S[(int64_t)t * a.ld + col] = s;
    }
}

// ---- which units does dropout keep?  (omc_mlp_dropout_masks: the device half of the mask oracle's known-answer test)
// Runs the very device functions the trainers and pass 2 call -- relu_dropout / _t / _n / _1 -- on activations of 1.0
// with each kernel's tags and its register -> hidden-unit map, and writes keep / drop per (layer, row, unit).
// variant 0: mlp_apply_kernel (key = path column, step = time step), 1: mlp_train_kernel, 2: mlp_train_tile_kernel,
// 3: mlp_train_quad_kernel (key = position in the minibatch, step = optimizer step).
template <int H>
__global__ __launch_bounds__(64) void mlp_mask_probe_kernel(int variant, int layers, int64_t n_rows, const uint32_t* keys,
                                                            uint32_t step, uint32_t keep16, float inv_keep, uint32_t k0,
                                                            uint32_t k1, uint8_t* __restrict__ out)
{
    constexpr int NT = H / 32;
    const int lane = threadIdx.x, c = lane & 31, h = lane >> 5;
    const int64_t row = (int64_t)blockIdx.x * 32 + c;
    if (row >= n_rows) return;
    const uint32_t key = keys ? keys[row] : (uint32_t)row;
    auto rho = [&](int r) { return (r >> 2) * 8 + 4 * h + (r & 3); };
    for (int j = 0; j < layers; ++j) {
        uint8_t* o = out + ((size_t)j * (size_t)n_rows + (size_t)row) * H;
        v16f z[NT];
#pragma unroll
        for (int mt = 0; mt < NT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) z[mt][r] = 1.0f;
        if (variant == 4) {  // 16-row tiles: lane (j, g) of wave w holds units 32 w + 8 g + 2 r + ub; here c <-> j, 16 rows per half-wave h
#pragma unroll
            for (int oct = 0; oct < H / 8; ++oct) {
                v4f16 zz[2] = {v4f16{1.0f, 1.0f, 1.0f, 1.0f}, v4f16{1.0f, 1.0f, 1.0f, 1.0f}};
                relu_dropout_q16(zz, key, step, 0x100u * (uint32_t)(j + 1) + (uint32_t)oct, keep16, inv_keep, k0, k1);
                if (h == 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        o[8 * oct + 2 * r] = zz[0][r] != 0.0f;
                        o[8 * oct + 2 * r + 1] = zz[1][r] != 0.0f;
                    }
                }
            }
            continue;
        }
        if (variant == 3) {
#pragma unroll
            for (int w = 0; w < NT; ++w) {
                relu_dropout_1(z[w], key, step, 0x100u * (uint32_t)(j + 1) + 0x10u * (uint32_t)w + (uint32_t)h, keep16,
                               inv_keep, k0, k1);
#pragma unroll
                for (int r = 0; r < 16; ++r) o[32 * w + rho(r)] = z[w][r] != 0.0f;
            }
            continue;
        }
        if constexpr (NT == 1) {
            if (variant == 0) {  // pass 2 with one 32-unit tile
                const uint32_t tag = (j == 0 ? 0x300u : 0x400u + 0x100u * (uint32_t)(j - 1)) + (uint32_t)h;
                relu_dropout_n<1>(z, key, step, tag, keep16, inv_keep, k0, k1);
#pragma unroll
                for (int r = 0; r < 16; ++r) o[unit_of(0, r, h)] = z[0][r] != 0.0f;
            }
        }
        if constexpr (NT >= 2) {
            if (variant == 2) {
                relu_dropout_t<NT, true>(z, key, step, 0x100u * (uint32_t)(j + 1) + (uint32_t)h, keep16, inv_keep, k0, k1);
#pragma unroll
                for (int mt = 0; mt < NT; ++mt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[NT * rho(r) + mt] = z[mt][r] != 0.0f;
            } else if (variant == 1) {
                if constexpr (NT == 2) {
                    relu_dropout<false>(z, key, step, 0x100u * (uint32_t)(j + 1) + (uint32_t)h, keep16, inv_keep, k0, k1);
#pragma unroll
                    for (int mt = 0; mt < NT; ++mt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) o[unit_of(mt, r, h)] = z[mt][r] != 0.0f;
                }
            } else {
                const uint32_t tag = (j == 0 ? 0x300u : 0x400u + 0x100u * (uint32_t)(j - 1)) + (uint32_t)h;
                relu_dropout_n<NT>(z, key, step, tag, keep16, inv_keep, k0, k1);
#pragma unroll
                for (int mt = 0; mt < NT; ++mt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[unit_of(mt, r, h)] = z[mt][r] != 0.0f;
            }
        }
    }
}

}  // namespace

hipError_t mlp_dropout_masks(hipStream_t st, int variant, int hidden, int layers, int64_t n_rows, const uint32_t* keys,
                             uint32_t step, uint64_t seed, double dropout, uint8_t* out)
{
    const DropKeep k = dropout_keep(dropout);
    return dispatch_h(hidden, [&](auto h) -> hipError_t {  // any of the three widths; `layers` is a run-time loop bound
        hipLaunchKernelGGL(mlp_mask_probe_kernel<decltype(h)::value>, dim3((unsigned)((n_rows + 31) / 32)), dim3(64), 0, st,
                           variant, layers, n_rows, keys, step, k.keep16, k.inv_keep, (uint32_t)seed, (uint32_t)(seed >> 32), out);
        return hipGetLastError();
    });
}

template <int H, int L>
static hipError_t launch_apply(hipStream_t st, const MlpApplyArgs& a)
{
    static std::atomic<uint64_t> attr_mask{0};  // per device (omc_kernels.h)
    const size_t lds_bytes = sizeof(float) * (size_t)apply_lds_floats(H, L);
    hipError_t e = set_max_dynamic_lds(attr_mask, reinterpret_cast<const void*>(mlp_apply_kernel<H, L>), lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((mlp_apply_kernel<H, L>), dim3((unsigned)((a.ntiles + 3) / 4)), dim3(256), lds_bytes, st, a);
    return hipGetLastError();
}

hipError_t mlp_apply_pass2(hipStream_t st, const LsmProblem& p, int hidden, int layers, const float* params,
                           const double* feat_mean, const double* feat_std, double y_mean, double y_std,
                           double dropout, uint64_t seed, float* sx, int32_t* tex, int64_t col_base0, int64_t col_base1)
{
    MlpApplyArgs a;
    a.key_half = p.M / 2; a.key_base0 = col_base0; a.key_base1 = col_base1;
    a.S = p.S; a.ld = p.ld; a.M = p.M; a.N = p.N; a.is_put = p.is_put;
    a.K = p.K; a.T = p.T; a.dt = p.T / (double)p.N;
    a.params = params;
    for (int i = 0; i < 7; ++i) {
        a.fm[i] = feat_mean[i];
        a.rs[i] = 1.0 / feat_std[i];
    }
    a.ym = y_mean; a.ysd = y_std;
    a.sx = sx; a.tex = tex;
    const DropKeep k = dropout_keep(dropout);
    a.keep16 = k.keep16; a.inv_keep = k.inv_keep;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    a.ntiles = (int)((p.M + 31) / 32);
    return dispatch_hl(hidden, layers, [&](auto h, auto l) {  // every shape of mlp_param_count
        return launch_apply<decltype(h)::value, decltype(l)::value>(st, a);
    });
}

int localvol_param_count(int hidden, int layers)
{
    if (hidden != 64 || layers < 1 || layers > 8) return -1;
    return kH * 4 + layers * (kH * kH + 3 * kH) + kH + 1;
}

hipError_t localvol_paths(hipStream_t st, float* S, int64_t ld, int64_t M, int N, int layers, const float* params,
                          const float* Z, double S0, double r, double T, double K, double m_scale,
                          double tau_scale, double eps_out)
{
    LocalVolArgs a;
    a.S = S; a.ld = ld; a.M = M; a.P = M / 2; a.N = N; a.L = layers;
    a.params = params; a.Z = Z;
    const double dt = T / (double)N;
    a.s0 = (float)S0; a.r = (float)r; a.dt = (float)dt; a.sqdt = (float)sqrt(dt); a.eps_out = (float)eps_out;
    a.K = K; a.T = T; a.dtd = dt; a.inv_m_scale = 1.0 / m_scale; a.inv_tau_scale = 1.0 / tau_scale;
    a.ntiles = (int)((M + 31) / 32);
    const size_t lds_bytes = sizeof(float) * (size_t)(kH * 4 + layers * (kH * kLdW2 + 3 * kH) + kH + 4);
    if (lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(localvol_paths_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(localvol_paths_kernel, dim3((unsigned)((a.ntiles + 3) / 4)), dim3(256), lds_bytes, st, a);
    return hipGetLastError();
}

}  // namespace omc
