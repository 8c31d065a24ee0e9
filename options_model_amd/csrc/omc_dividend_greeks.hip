// omc_dividend_greeks.hip -- frozen-policy pathwise Greeks of American options on a stock that pays discrete dividends
// (the definitions are in include/omc_dividend_greeks.h).
//
// A cash dividend makes the stored spot affine in S0, not linear: omc_greeks.hip's "stored path times lambda" scenarios
// and its ln(s / S0) Brownian value do not exist here.  dividend_greeks_kernel<MODEL, PUT> REGENERATES the paths instead:
// one lane per antithetic pair walks forward through dividend_paths_kernel<MODEL, 1>'s loop -- same Philox counters, same
// normals4 blocks, same model step, same scalar "next dividend entry" test, same fmaxf(fmaf(s, mul, -cash), 0) -- and reads
// no path matrix.  Per partner it carries three float32 SCENARIO spots, started at (float)S0, (float)(S0 (1 + h)) and
// (float)(S0 (1 - h)) and driven by the same growth factor G of the step (G depends on no spot: one exp2 and, under
// Heston, one variance update serve all three; omc_paths_dev.h, heston_pair_factors).  Six CHAINS per lane, each deciding
// with the same frozen fits (LDS, fits_to_lds) by pass 2's expression on its own spot in float64.  A chain's exercise step
// is the one pass 2 keeps: the LATEST step in 1 .. N-1 at which the rule fires, else N (pass 2 and omc_greeks.hip walk
// backward and stop at the first fire they meet).  Walking forward, a chain copies its running state -- spot and
// tangents -- at every fire and takes step N's when it has never fired, as omc_basket_greeks.hip; so every lane walks all
// N steps.
//
// Tangents, stepped with the spot (eps = +-1 the partner, Sm = S G the cum-dividend spot):
//   every scenario   Y  <- Y G, Y_0 = 1                                         dS/dS0 of that scenario
//   GBM, base only   Ys <- Ys G + Sm (-sigma dt + eps sqrt(dt) z)               dS/dsigma
//                    Yr <- Yr G + Sm dt                                         dS/dr  (dS/dq = -Yr)
//                    YT <- YT G + Sm ((r - q - sigma^2/2)/N + eps sigma z / (2 sqrt(T N)))   dS/dT at fixed N
// and on a dividend step every tangent becomes mul Y where the ex-dividend spot is positive, 0 where the floor took it.
// All Greek terms are formed once, after the walk, in omc_greeks.hip's three groups of 8 sums (epsilon in its two free
// slots) through block_reduce8; per-workgroup partials in a fixed order, then one finalize launch: two identical calls
// return identical bits.  Every loop over chains unrolls and no array is indexed at run time: no scratch
// (profiles/dividend_greeks_resource_usage.txt).
#include "omc_dividend_greeks.h"

#include "omc_lsm_dev.h"
#include "omc_paths_dev.h"

namespace omc {

// the float32 constants of the GBM tangents' source terms
struct DivTangentC {
    float sig_a, sig_b;  // -sigma dt, sqrt(dt)
    float dt;
    float T_a, T_b;      // (r - q - sigma^2/2) / N, sigma / (2 sqrt(T N))
};

struct DivGreeksKArgs {
    PathArgs g;           // the generator's argument block (S, ld unused)
    float s_up, s_dn;     // (float)(S0 (1 + h)), (float)(S0 (1 - h))
    DivTangentC tc;
    int is_put;
    double K, S0, r, T, h;
    const DivEntry* tab;
    const double* D;
    const double* betas;
    double* part;
};

// one partner's chains: scenario c = 0 base, 1 up, 2 down.  The running state steps on; the chain's own state is the
// running one at the LATEST step in 1 .. N-1 at which the rule fired, else at step N
struct DivChains {
    float s[3], Y[3];      // running: the scenario's spot and dS/dS0
    float Ys, Yr, YT;      // running, GBM, base scenario
    float sx[3], Yx[3];    // the chain's: at its exercise step
    float Ysx, Yrx, YTx;
    int k[3];              // the chain's exercise step; N while the rule has not fired
};

// MODEL 0 GBM, 1/2/3/4 Heston scheme 0/1/2/3
template <int MODEL>
__device__ __forceinline__ float grow(float s, float G)
{
    if constexpr (MODEL == 0) return s * G;
    else return heston_grow<MODEL - 1>(s, G);
}

// one partner through one step: the model's step on every scenario, the dividend of the step, the decisions
template <int MODEL, int PUT>
__device__ __forceinline__ void chains_step(const DivGreeksKArgs& a, DivChains& ch, float G, float ez, int t, bool div,
                                            const DivEntry& e, const Fit& f, double invK)
{
    const int N = a.g.n_steps;
    const bool last = t == N;
    if constexpr (MODEL == 0) {  // (on the cum-dividend spot of the base scenario)
        const float sm = ch.s[0] * G;
        ch.Ys = __builtin_fmaf(sm, __builtin_fmaf(a.tc.sig_b, ez, a.tc.sig_a), ch.Ys * G);
        ch.Yr = __builtin_fmaf(sm, a.tc.dt, ch.Yr * G);
        ch.YT = __builtin_fmaf(sm, __builtin_fmaf(a.tc.T_b, ez, a.tc.T_a), ch.YT * G);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float s = grow<MODEL>(ch.s[c], G);  // the cum-dividend spot
        float Y = grow<MODEL>(ch.Y[c], G);
        if (div) {  // wave-uniform
            s = __builtin_fmaxf(__builtin_fmaf(s, e.mul, -e.cash), 0.0f);
            const float m = s > 0.0f ? e.mul : 0.0f;
            Y = m * Y;
            if (MODEL == 0 && c == 0) {
                ch.Ys = m * ch.Ys;
                ch.Yr = m * ch.Yr;
                ch.YT = m * ch.YT;
            }
        }
        ch.s[c] = s;
        ch.Y[c] = Y;
        // (a step without a fit -- t = N among them -- has b0 = +inf: the rule does not fire; step N is the chain's when it
        // never has)
        const bool ex = exercises(pay_stored((double)s, a.K, invK, PUT), f) | (last & (ch.k[c] == N));
        ch.k[c] = ex ? t : ch.k[c];
        ch.sx[c] = ex ? s : ch.sx[c];
        ch.Yx[c] = ex ? Y : ch.Yx[c];
        if (MODEL == 0 && c == 0) {
            ch.Ysx = ex ? ch.Ys : ch.Ysx;
            ch.Yrx = ex ? ch.Yr : ch.Yrx;
            ch.YTx = ex ? ch.YT : ch.YTx;
        }
    }
}

template <int MODEL, int PUT>
__global__ __launch_bounds__(kBlock) void dividend_greeks_kernel(DivGreeksKArgs a)
{
    extern __shared__ double sh_b[];  // [N+1][4]: b0, b1, b2 (b0 = +inf: no exercise at t)
    __shared__ double red[kNQ * kRedStride];
    const int tid = threadIdx.x;
    const int N = a.g.n_steps;
    fits_to_lds<false>(sh_b, nullptr, nullptr, a.betas, nullptr, N);
    const double K = a.K, invK = 1.0 / a.K;
    const int64_t p = (int64_t)blockIdx.x * kBlock + tid;
    const bool valid = p < a.g.P;

    DivChains ca, cb;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ca.s[c] = cb.s[c] = c == 0 ? a.g.s_init : c == 1 ? a.s_up : a.s_dn;
        ca.Y[c] = cb.Y[c] = 1.0f;
        ca.sx[c] = cb.sx[c] = ca.Yx[c] = cb.Yx[c] = 0.0f;
        ca.k[c] = cb.k[c] = N;
    }
    ca.Ys = ca.Yr = ca.YT = cb.Ys = cb.Yr = cb.YT = 0.0f;
    ca.Ysx = ca.Yrx = ca.YTx = cb.Ysx = cb.Yrx = cb.YTx = 0.0f;
    float va = a.g.v_init, vb = a.g.v_init;

    constexpr int SPB = MODEL == 0 ? 4 : 2;  // steps per Philox block of normals
    const int nblk = (N + SPB - 1) / SPB;
    const uint64_t pair = a.g.pair_offset + (uint64_t)(valid ? p : 0);
    DivEntry e = a.tab[0];  // the next dividend step: the same for every lane
    int next = 1;
    int t = 0;
    for (int blk = 0; blk < nblk; ++blk) {
        float z[4];
        normals4(pair, (uint32_t)blk, a.g.stream, a.g.k0, a.g.k1, z);
#pragma unroll
        for (int i = 0; i < SPB; ++i) {
            if (++t > N) break;
            float Ga, Gb, ez;
            if constexpr (MODEL == 0) {
                ez = z[i];
                Ga = fast_exp2(__builtin_fmaf(a.g.b, z[i], a.g.a));
                Gb = fast_exp2(__builtin_fmaf(-a.g.b, z[i], a.g.a));
            } else {
                ez = 0.0f;
                heston_pair_factors<MODEL - 1>(a.g.hc, z[2 * i], z[2 * i + 1], va, vb, Ga, Gb);
            }
            const bool div = t == e.step;
            const Fit f = fit_lds(sh_b, t);
            chains_step<MODEL, PUT>(a, ca, Ga, ez, t, div, e, f, invK);
            chains_step<MODEL, PUT>(a, cb, Gb, -ez, t, div, e, f, invK);
            if (div) e = a.tab[next++];
        }
    }

    // ---- the per-path terms, from the chains' own states alone
    double g0[kNQ], g1[kNQ], g2[kNQ];
#pragma unroll
    for (int q = 0; q < kNQ; ++q) g0[q] = g1[q] = g2[q] = 0.0;
    if (valid) {
        const double sign = PUT ? -1.0 : 1.0;
        const double dt = a.T / N, r = a.r;
        auto partner = [&](const DivChains& ch) {
            const int k = ch.k[0];
            const double imm = payoff_d(ch.sx[0], K, PUT);
            const double Dk = a.D[k - 1];
            const double cf = add_cash_flow(g0, imm, Dk, k < N);  // the pricing's cash-flow, bit for bit
            const double Dp = (imm > 0.0 ? sign : 0.0) * Dk;      // D_k phi'(s)
            const double delta = Dp * (double)ch.Yx[0];
            g1[0] += delta;
            g1[1] += delta * delta;
            if constexpr (MODEL == 0) {
                const double vega = Dp * (double)ch.Ysx;
                const double eps = -Dp * (double)ch.Yrx;
                const double rho = -(k - 1) * dt * cf - eps;
                const double theta = -(-r * (k - 1) / N * cf + Dp * (double)ch.YTx);
                g1[4] += vega;
                g1[5] += vega * vega;
                g1[6] += rho;
                g1[7] += rho * rho;
                g2[0] += theta;
                g2[1] += theta * theta;
                g2[4] += eps;
                g2[5] += eps * eps;
            }
            double dlt[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int ke = ch.k[1 + s];
                const double ie = payoff_d(ch.sx[1 + s], K, PUT);
                const double De = a.D[ke - 1];
                g0[5 + s] += (ie > 0.0 ? ie : 0.0) * De;
                g2[2 + s] += ke < N ? 1.0 : 0.0;
                dlt[s] = (ie > 0.0 ? sign : 0.0) * De * (double)ch.Yx[1 + s];
            }
            const double gamma = (dlt[0] - dlt[1]) / (2.0 * a.h * a.S0);
            g1[2] += gamma;
            g1[3] += gamma * gamma;
        };
        partner(ca);
        partner(cb);
    }
    // three 8-quantity block reductions through one LDS patch; partials [kGreeksQ][nwg]
    const size_t nwg = gridDim.x;
    double s = block_reduce8(g0, red);
    if (tid < 64 && (tid & 7) == 0) a.part[(size_t)(tid >> 3) * nwg + blockIdx.x] = s;
    __syncthreads();
    s = block_reduce8(g1, red);
    if (tid < 64 && (tid & 7) == 0) a.part[(size_t)(8 + (tid >> 3)) * nwg + blockIdx.x] = s;
    __syncthreads();
    s = block_reduce8(g2, red);
    if (tid < 64 && (tid & 7) == 0) a.part[(size_t)(16 + (tid >> 3)) * nwg + blockIdx.x] = s;
}

// workgroup g adds quantities 8g .. 8g+7 over the sweep's partials (workgroup order fixed); slot 4 = the regression-set sizes
__global__ __launch_bounds__(kBlock) void dividend_greeks_finalize_kernel(const double* __restrict__ part, int64_t nwg,
                                                                          const double* __restrict__ gmom, int N,
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
    if (g == 0 && gmom) {
        for (int t = 1 + tid; t < N; t += kBlock) acc[4] += gmom[(size_t)t * 8];
    }
    const double s = block_reduce8(acc, red);
    if (tid < 64 && (tid & 7) == 0) result[8 * g + (tid >> 3)] = s;
}

int64_t dividend_greeks_blocks(int64_t n_paths)
{
    return (n_paths / 2 + kBlock - 1) / kBlock;
}

hipError_t dividend_greeks(hipStream_t st, const DivGreeksArgs& a, hipEvent_t ev_begin, hipEvent_t ev_end)
{
    const PathSpec& s = a.paths;
    const int64_t P = s.n_paths / 2;
    const int N = s.n_steps;
    if (P <= 0 || N < 1 || N > kMaxSteps) return hipErrorInvalidValue;
    DivGreeksKArgs k{};
    k.g = make_path_args(s, P);
    const double S0 = s.S0, dt = s.T / N;
    k.s_up = (float)(S0 * (1.0 + a.h));
    k.s_dn = (float)(S0 * (1.0 - a.h));
    k.tc.sig_a = (float)(-s.sigma * dt);
    k.tc.sig_b = (float)std::sqrt(dt);
    k.tc.dt = (float)dt;
    k.tc.T_a = (float)((s.r - 0.5 * s.sigma * s.sigma) / N);  // (s.r is the drift rate r - q)
    k.tc.T_b = (float)(s.sigma / (2.0 * std::sqrt(s.T * N)));
    k.is_put = a.is_put ? 1 : 0;
    k.K = a.K; k.S0 = S0; k.r = a.r; k.T = s.T; k.h = a.h;
    k.tab = a.tab; k.D = a.D; k.betas = a.betas; k.part = a.part;
    const int64_t nwg = dividend_greeks_blocks(s.n_paths);
    const size_t dyn = sizeof(double) * 4 * (size_t)(N + 1);
    if (ev_begin) (void)hipEventRecord(ev_begin, st);
    for_model(s.model, s.scheme, [&](auto model) {
        for_put(k.is_put, [&](auto put) {
            constexpr int MO = decltype(model)::value, PUT = decltype(put)::value;
            hipLaunchKernelGGL((dividend_greeks_kernel<MO, PUT>), dim3((unsigned)nwg), dim3(kBlock), dyn, st, k);
        });
    });
    if (ev_end) (void)hipEventRecord(ev_end, st);
    hipLaunchKernelGGL(dividend_greeks_finalize_kernel, dim3(3), dim3(kBlock), 0, st, a.part, nwg, a.gmom, N, a.result);
    return hipGetLastError();
}

}  // namespace omc
