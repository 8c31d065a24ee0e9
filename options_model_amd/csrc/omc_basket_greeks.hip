// omc_basket_greeks.hip -- frozen-policy pathwise Greeks of American options on the index of D correlated GBM assets
// (the definitions are in include/omc.h).
//
// basket_greeks_kernel<D, GAMMA, PUT>: one lane per antithetic pair, no grid-stride loop.  The lane REGENERATES both
// partners' D assets forward with the generator's own helpers (omc_basket_dev.h: same counters, same operations, same
// bits as the stored matrices -- it reads no path matrix) and forms the index from the same registers.  Per partner it
// follows 2 D + 1 CHAINS: the base pricing (pass 2's very expressions on the float32 index) and, with GAMMA, asset i
// scaled by 1 + h and by 1 - h, each deciding with the same frozen fits (LDS, fits_to_lds) on its own float64 index.  A
// chain's exercise step is the LATEST step in 1 .. N-1 at which the rule fires, else N: walking forward, a chain
// overwrites its small state at every fire, and takes step N's when it has never fired.  State of a chain:
//   base        the D asset spots, the index, the step
//   scenario    two floats and a 16-bit step (the up and down steps of an asset share a register):
//               arithmetic (X, s_i), best-of / worst-of (wf_i * s_i, the max / min of the OTHER assets' products),
//               geometric (g, -) -- the scenario's index and its partial are functions of these (scen_index, scen_x)
// All Greek terms are formed once, after the last step, in groups of 8 sums (omc_basket_greeks.h) that go through
// block_reduce8 one after the other; a finalize launch adds the per-workgroup partials in workgroup order: two identical
// calls return identical bits.
// The kind is wave-uniform (the law comes by value): one scalar branch selects the body of the kind.  D, GAMMA and PUT are
// template parameters, every loop over assets, scenarios and partners unrolls, no array is indexed at run time: no
// scratch in any instantiation (profiles/basket_greeks_resource_usage.txt).
#include "omc_basket_greeks.h"

#include "omc_basket_dev.h"
#include "omc_lsm_dev.h"

namespace omc {

template <int D>
struct GreekChains {
    float s[D], x;            // base chain: the asset spots and the index at its exercise step
    int k;                    // its step
    float A[D][2], B[D][2];   // scenario chain (asset i; 0 up, 1 down): its two floats
    uint32_t kk[D];           // their steps: up in the low 16 bits, down in the high ones (N <= kMaxSteps < 2^16)
};

// the float64 index of the scenario "asset i scaled by 1 + h (e = 0) or 1 - h (e = 1)" from the chain's two floats
template <int KIND>
__device__ __forceinline__ double scen_index(const BasketGreeksArgs& a, int i, int e, float A, float B)
{
    if constexpr (KIND == OMC_BASKET_ARITHMETIC) return fma(e ? -a.hw[i] : a.hw[i], (double)B, (double)A);
    else if constexpr (KIND == OMC_BASKET_GEOMETRIC) return (double)A * (e ? a.cdn[i] : a.cup[i]);
    else if constexpr (KIND == OMC_BASKET_BEST_OF) return fmax((e ? a.ldn : a.lup) * (double)A, (double)B);
    else return fmin((e ? a.ldn : a.lup) * (double)A, (double)B);
}
// its partial dX/ds_i s_i, unscaled: of the scenario's own argmax (the scaled asset carries the index on a tie)
template <int KIND>
__device__ __forceinline__ double scen_x(const BasketGreeksArgs& a, const BasketLaw& c, int i, int e, float A, float B)
{
    if constexpr (KIND == OMC_BASKET_ARITHMETIC) return (double)c.w[i] * (double)B;
    else if constexpr (KIND == OMC_BASKET_GEOMETRIC) return (double)c.w[i] * (double)A;
    else if constexpr (KIND == OMC_BASKET_BEST_OF) return (e ? a.ldn : a.lup) * (double)A >= (double)B ? (double)A : 0.0;
    else return (e ? a.ldn : a.lup) * (double)A <= (double)B ? (double)A : 0.0;
}

// one partner at step t: every chain decides on its index and overwrites its state where it fires (step N: where it
// never has)
template <int KIND, int D, bool GAMMA, int PUT>
__device__ __forceinline__ void greek_decide(const BasketGreeksArgs& a, const BasketLaw& c, const float (&s)[D], float X, int t,
                                             const Fit& f, GreekChains<D>& ch)
{
    const int N = a.N;
    const bool last = t == N;
    {
        const bool ex = exercises(pay_stored((double)X, a.K, a.invK, PUT), f) | (last & (ch.k == N));
        ch.k = ex ? t : ch.k;
        ch.x = ex ? X : ch.x;
#pragma unroll
        for (int i = 0; i < D; ++i) ch.s[i] = ex ? s[i] : ch.s[i];
    }
    if constexpr (GAMMA) {
        float A[D], B[D];
        if constexpr (KIND == OMC_BASKET_ARITHMETIC || KIND == OMC_BASKET_GEOMETRIC) {
#pragma unroll
            for (int i = 0; i < D; ++i) {
                A[i] = X;
                B[i] = s[i];
            }
        } else {  // the float32 products the index compares, and for each asset the extreme of the others'
            constexpr bool BEST = KIND == OMC_BASKET_BEST_OF;
            const float none = BEST ? -__builtin_inff() : __builtin_inff();
            float pre[D], suf[D];
#pragma unroll
            for (int i = 0; i < D; ++i) A[i] = c.w[i] * s[i];
            pre[0] = none;
#pragma unroll
            for (int i = 1; i < D; ++i) pre[i] = BEST ? fmaxf(pre[i - 1], A[i - 1]) : fminf(pre[i - 1], A[i - 1]);
            suf[D - 1] = none;
#pragma unroll
            for (int i = D - 2; i >= 0; --i) suf[i] = BEST ? fmaxf(suf[i + 1], A[i + 1]) : fminf(suf[i + 1], A[i + 1]);
#pragma unroll
            for (int i = 0; i < D; ++i) B[i] = BEST ? fmaxf(pre[i], suf[i]) : fminf(pre[i], suf[i]);
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const double Xs = scen_index<KIND>(a, i, e, A[i], B[i]);
                const uint32_t ke = e ? ch.kk[i] >> 16 : ch.kk[i] & 0xffffu;
                const bool ex = exercises(pay_stored(Xs, a.K, a.invK, PUT), f) | (last & (ke == (uint32_t)N));
                ch.A[i][e] = ex ? A[i] : ch.A[i][e];
                if constexpr (KIND != OMC_BASKET_GEOMETRIC) ch.B[i][e] = ex ? B[i] : ch.B[i][e];
                const uint32_t kn = e ? (ch.kk[i] & 0xffffu) | ((uint32_t)t << 16) : (ch.kk[i] & 0xffff0000u) | (uint32_t)t;
                ch.kk[i] = ex ? kn : ch.kk[i];
            }
        }
    }
}

// what the per-asset groups reuse of a partner's base chain
struct GreekBase {
    double Dp, tk;  // D_k phi'(X); k dt
    uint32_t carrier;  // best-of / worst-of: bit i set = asset i is the lowest one whose float32 product is the index
};

// x_i = dX/ds_i s_i of the base chain
template <int KIND, int D>
__device__ __forceinline__ double base_x(const BasketLaw& c, const GreekChains<D>& ch, const GreekBase& b, int i)
{
    if constexpr (KIND == OMC_BASKET_ARITHMETIC) return (double)c.w[i] * (double)ch.s[i];
    else if constexpr (KIND == OMC_BASKET_GEOMETRIC) return (double)c.w[i] * (double)ch.x;
    else return (b.carrier >> i) & 1u ? (double)(c.w[i] * ch.s[i]) : 0.0;
}

template <int KIND, int D, bool GAMMA, int PUT>
__device__ __forceinline__ void basket_greeks_body(const BasketGreeksArgs& a, const BasketLaw& c, const double* sh_b, double* red)
{
    const int tid = threadIdx.x;
    const int N = a.N;
    const int64_t p = (int64_t)blockIdx.x * kBlock + tid;
    const bool valid = p < a.P;
    constexpr bool GEO = KIND == OMC_BASKET_GEOMETRIC;

    GreekChains<D> cha, chb;
    cha.k = chb.k = N;
    cha.x = chb.x = 0.0f;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        cha.s[i] = chb.s[i] = 0.0f;
        cha.kk[i] = chb.kk[i] = (uint32_t)N | ((uint32_t)N << 16);
#pragma unroll
        for (int e = 0; e < 2; ++e) cha.A[i][e] = cha.B[i][e] = chb.A[i][e] = chb.B[i][e] = 0.0f;
    }

    if (valid) {
        float sa[D], sb[D], ga = c.g0, gb = c.g0;
#pragma unroll
        for (int i = 0; i < D; ++i) sa[i] = sb[i] = c.s0[i];
        const uint64_t pair = a.pair_offset + (uint64_t)p;
        const int nblk = (N + 3) >> 2;
        int t = 0;
        for (int blk = 0; blk < nblk; ++blk) {
            float y[D][4];
            basket_normals<D>(c, pair, (uint32_t)blk, a.stream, a.k0, a.k1, y);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (++t > N) break;
                float xa, xb;
                if constexpr (GEO) {  // the generator's rule: the state steps with the weighted exponents
                    float E = 0.0f, Eb = 0.0f;
#pragma unroll
                    for (int i = 0; i < D; ++i) {
                        const float e = __builtin_fmaf(c.b[i], y[i][u], c.a[i]);
                        const float eb = __builtin_fmaf(-c.b[i], y[i][u], c.a[i]);
                        sa[i] = sa[i] * fast_exp2(e);
                        sb[i] = sb[i] * fast_exp2(eb);
                        E = i == 0 ? c.w[0] * e : __builtin_fmaf(c.w[i], e, E);
                        Eb = i == 0 ? c.w[0] * eb : __builtin_fmaf(c.w[i], eb, Eb);
                    }
                    ga = ga * fast_exp2(E);
                    gb = gb * fast_exp2(Eb);
                    xa = ga;
                    xb = gb;
                } else {
                    basket_step<D>(c, sa, sb, y, u);
                    xa = basket_index<KIND, D>(c, sa);
                    xb = basket_index<KIND, D>(c, sb);
                }
                const Fit f = fit_lds(sh_b, t);
                greek_decide<KIND, D, GAMMA, PUT>(a, c, sa, xa, t, f, cha);
                greek_decide<KIND, D, GAMMA, PUT>(a, c, sb, xb, t, f, chb);
            }
        }
    }

    // ---- the per-path terms, from the chains' states alone, in groups of 8 sums
    const size_t nwg = gridDim.x;
    const double sign = PUT ? -1.0 : 1.0;
    const double K = a.K, dt = a.T / N, r = a.r, T = a.T;
    int group = 0;
    auto reduce_group = [&](const double (&g)[kNQ]) {
        const double s = block_reduce8(g, red);
        if (tid < 64 && (tid & 7) == 0) a.part[(size_t)(8 * group + (tid >> 3)) * nwg + blockIdx.x] = s;
        __syncthreads();
        ++group;
    };

    GreekBase ba{0.0, 0.0, 0u}, bb{0.0, 0.0, 0u};
    {
        double g[kNQ];
#pragma unroll
        for (int q = 0; q < kNQ; ++q) g[q] = 0.0;
        auto partner = [&](const GreekChains<D>& ch, GreekBase& b) {
            {
                const int k = ch.k;
                const double Dk = a.D[k - 1];
                const double imm = payoff_d(ch.x, K, PUT);
                const double cf = add_cash_flow(g, imm, Dk, k < N);  // the pricing's cash-flow, bit for bit
                b.Dp = (imm > 0.0 ? sign : 0.0) * Dk;
                b.tk = k * dt;
                if constexpr (KIND == OMC_BASKET_BEST_OF || KIND == OMC_BASKET_WORST_OF) {
#pragma unroll
                    for (int i = 0; i < D; ++i) b.carrier |= (b.carrier == 0u && c.w[i] * ch.s[i] == ch.x) ? 1u << i : 0u;
                }
                double sumx = 0.0, sumth = 0.0;
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    const double x = base_x<KIND, D>(c, ch, b, i);
                    const double lnr = log((double)ch.s[i] / a.S0[i]);
                    sumx += x;
                    sumth += x * (lnr + (r - a.q[i] - 0.5 * a.sigma[i] * a.sigma[i]) * b.tk);
                }
                const double rho = -(k - 1) * dt * cf + b.Dp * b.tk * sumx;
                const double theta = -(-r * (k - 1) * dt / T * cf + b.Dp * sumth / (2.0 * T));
                g[4] += rho;
                g[5] += rho * rho;
                g[6] += theta;
                g[7] += theta * theta;
            }
        };
        if (valid) {
            partner(cha, ba);
            partner(chb, bb);
        }
        reduce_group(g);
    }
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double g[kNQ];
#pragma unroll
        for (int q = 0; q < kNQ; ++q) g[q] = 0.0;
        auto partner = [&](const GreekChains<D>& ch, const GreekBase& b) {
            {
                const double x = base_x<KIND, D>(c, ch, b, i);
                const double lnr = log((double)ch.s[i] / a.S0[i]);
                const double delta = b.Dp * x / a.S0[i];
                const double vega = b.Dp * x * (lnr - (r - a.q[i] + 0.5 * a.sigma[i] * a.sigma[i]) * b.tk) / a.sigma[i];
                g[0] += delta;
                g[1] += delta * delta;
                g[2] += vega;
                g[3] += vega * vega;
                if constexpr (GAMMA) {
                    double dlt[2];
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int ke = (int)(e ? ch.kk[i] >> 16 : ch.kk[i] & 0xffffu);
                        const double Xs = scen_index<KIND>(a, i, e, ch.A[i][e], ch.B[i][e]);
                        const double ie = PUT ? K - Xs : Xs - K;
                        const double De = a.D[ke - 1];
                        g[6 + e] += (ie > 0.0 ? ie : 0.0) * De;
                        dlt[e] = (ie > 0.0 ? sign : 0.0) * De * scen_x<KIND>(a, c, i, e, ch.A[i][e], ch.B[i][e]) / a.S0[i];
                    }
                    const double gamma = (dlt[0] - dlt[1]) / (2.0 * a.h * a.S0[i]);
                    g[4] += gamma;
                    g[5] += gamma * gamma;
                }
            }
        };
        if (valid) {
            partner(cha, ba);
            partner(chb, bb);
        }
        reduce_group(g);
    }
#pragma unroll
    for (int j0 = 0; j0 < 2 * D; j0 += 8) {  // the scenario chains' early exercises
        double g[kNQ];
#pragma unroll
        for (int q = 0; q < kNQ; ++q) {
            g[q] = 0.0;
            const int i = (j0 + q) >> 1, e = (j0 + q) & 1;
            if (GAMMA && i < D && valid) {
                const int ka = (int)(e ? cha.kk[i < D ? i : 0] >> 16 : cha.kk[i < D ? i : 0] & 0xffffu);
                const int kb = (int)(e ? chb.kk[i < D ? i : 0] >> 16 : chb.kk[i < D ? i : 0] & 0xffffu);
                g[q] = (ka < N ? 1.0 : 0.0) + (kb < N ? 1.0 : 0.0);
            }
        }
        reduce_group(g);
    }
}

template <int D, bool GAMMA, int PUT>
__global__ __launch_bounds__(kBlock) void basket_greeks_kernel(BasketGreeksArgs a, BasketLaw c)
{
    extern __shared__ double sh_b[];  // [N+1][4]: b0, b1, b2 (b0 = +inf: no exercise at t)
    __shared__ double red[kNQ * kRedStride];
    fits_to_lds<false>(sh_b, nullptr, nullptr, a.betas, nullptr, a.N);
    if (c.kind == OMC_BASKET_ARITHMETIC) basket_greeks_body<OMC_BASKET_ARITHMETIC, D, GAMMA, PUT>(a, c, sh_b, red);
    else if (c.kind == OMC_BASKET_GEOMETRIC) basket_greeks_body<OMC_BASKET_GEOMETRIC, D, GAMMA, PUT>(a, c, sh_b, red);
    else if (c.kind == OMC_BASKET_BEST_OF) basket_greeks_body<OMC_BASKET_BEST_OF, D, GAMMA, PUT>(a, c, sh_b, red);
    else basket_greeks_body<OMC_BASKET_WORST_OF, D, GAMMA, PUT>(a, c, sh_b, red);
}

// workgroup g adds sums 8g .. 8g+7 over the sweep's partials, workgroup order fixed
__global__ __launch_bounds__(kBlock) void basket_greeks_finalize_kernel(const double* __restrict__ part, int64_t nwg,
                                                                        double* __restrict__ result)
{
    __shared__ double red[kNQ * kRedStride];
    const int tid = threadIdx.x, g = blockIdx.x;
    double acc[kNQ];
#pragma unroll
    for (int q = 0; q < kNQ; ++q) acc[q] = 0.0;
    for (int64_t i = tid; i < nwg; i += kBlock) {
#pragma unroll
        for (int q = 0; q < kNQ; ++q) acc[q] += part[(size_t)(8 * g + q) * nwg + i];
    }
    const double s = block_reduce8(acc, red);
    if (tid < 64 && (tid & 7) == 0) result[8 * g + (tid >> 3)] = s;
}

hipError_t basket_greeks(hipStream_t st, const BasketGreeksArgs& a, const BasketLaw& law, hipEvent_t ev_begin,
                         hipEvent_t ev_end)
{
    if (a.d < 1 || a.d > kBasketMax || a.P <= 0 || a.N < 1 || a.N > kMaxSteps) return hipErrorInvalidValue;
    const int64_t nwg = basket_greeks_blocks(a.P);
    const size_t dyn = sizeof(double) * 4 * (size_t)(a.N + 1);
    if (ev_begin) (void)hipEventRecord(ev_begin, st);
    for_assets(a.d, [&](auto d) {
        for_flag(a.want_gamma != 0, [&](auto gamma) {
            for_put(a.is_put, [&](auto put) {
                constexpr int DD = decltype(d)::value, PUT = decltype(put)::value;
                hipLaunchKernelGGL((basket_greeks_kernel<DD, decltype(gamma)::value, PUT>), dim3((unsigned)nwg), dim3(kBlock),
                                   dyn, st, a, law);
            });
        });
    });
    if (ev_end) (void)hipEventRecord(ev_end, st);
    hipLaunchKernelGGL(basket_greeks_finalize_kernel, dim3(basket_greeks_groups(a.d)), dim3(kBlock), 0, st, a.part, nwg,
                       a.result);
    return hipGetLastError();
}

}  // namespace omc
