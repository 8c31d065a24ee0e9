// omc_jump_greeks.hip -- frozen-policy Greeks of American options under jump-diffusion: Merton (GBM) and Bates (Heston)
// (the definitions are in include/omc_jump_greeks.h).
//
// With jumps ln(s / S0) holds the Brownian value AND the sum of the jump sizes: omc_greeks.hip cannot read the Brownian
// value back from a stored spot.  jump_greeks_kernel<MODEL, PUT> REGENERATES the paths instead: one lane per antithetic
// pair walks forward through jump_paths_kernel<MODEL, 1>'s loop -- same Philox counters for the normals, the count block
// (one per four steps) and the size block, same n = #{w >= thr[k]}, same jump_log2 -- and reads no path matrix.  The step
// keeps the generator's shape: one compare against thr[0] per pair, a ballot over the wave and a scalar branch go
// around everything a jump needs (the other 15 compares, the size block, the running jump sums and, under Heston, the
// extra exp2).  Per partner it carries three float32 SCENARIO spots, started at (float)S0, (float)(S0 (1 + h)) and
// (float)(S0 (1 - h)) and driven by ONE growth factor per step (GBM exp2(fma(+-b, z, a) + jl); Heston
// heston_pair_factors / heston_grow, then exp2(jl)).  Six CHAINS per lane decide with the frozen fits (LDS,
// fits_to_lds) by pass 2's expression on their own spot in float64; a chain's step is the one pass 2 keeps, the LATEST
// fire in 1 .. N-1, else N (section 32.1), so every lane walks all N steps and a chain copies its state at every fire.
//
// The spot is multiplicative in S0 and in every step's factor: no tangent recurrence.  gamma alone takes the bumped chains'
// dS/dS0 from ONE float32 product Y of the partner's growth factors (omc_dividend_greeks.hip's Y without dividends), not
// from s / (S0 (1 +- h)): the two quotients round differently, and their difference over 2 h S0 is float32 noise of the
// size of gamma itself on every path whose bumped chains stop together, where the term is exactly 0.  A pair carries
// three running sums, captured with the base chain's state at each fire:
//   Z_k  = sum_{j<=k} z_j  (W_k = sqrt(dt) Z_k; the partner's with the opposite sign)
//   Nc_k = sum_{j<=k} n_j  (integer)          ZJ_k = sum_{j<=k} sqrt(n_j) z_{J,j}
// Nc and ZJ change inside the jump branch only; Nc after step N is the pair's whole-path count N_tot.  The score terms
// of dlambda and theta use N_tot, not Nc_k: k is the latest fire and no stopping time, so only the full path's
// likelihood ratio is valid.  They are the derivatives of prod_j Poisson(n_j; x), x = lambda T / N, in lambda and in T:
// N_tot / lambda - T and N_tot / T - lambda.  The sampled law is the 24-bit quantised one, truncated at 16 jumps; its
// score differs from this one by O(2^-24) per step, far below any standard error.
//
// All Greek terms are formed once, after the walk, in float64: omc_greeks.hip's three groups of 8 sums (epsilon and the
// jump count in free slots) and a fourth group for the jump Greeks, through block_reduce8; per-workgroup partials in a
// fixed order, then one finalize launch: two identical calls return identical bits.  Every loop over chains unrolls and
// no array is indexed at run time: no scratch (profiles/jump_greeks_resource_usage.txt).
#include "omc_jump_greeks.h"

#include "omc_jump_dev.h"
#include "omc_lsm_dev.h"
#include "omc_paths_dev.h"

namespace omc {

struct JumpGreeksKArgs {
    PathArgs g;        // the generator's argument block (S, ld unused)
    JumpLaw law;
    float s_up, s_dn;  // (float)(S0 (1 + h)), (float)(S0 (1 - h))
    int is_put;
    double K, S0, r, T, h;
    double sigma, rj;                // rj: the generator's drift rate
    double lambda, sigma_j, kappa, kappa1;  // kappa1 = kappa + 1 = exp(mu_j + sigma_j^2 / 2)
    const double* D;
    const double* betas;
    double* part;
};

// one partner's chains: scenario c = 0 base, 1 up, 2 down.  The running spots step on; the chain's own state is the
// running one at the LATEST step in 1 .. N-1 at which the rule fired, else at step N
struct JumpChains {
    float s[3];   // running: the scenario's spot
    float sx[3];  // the chain's: at its exercise step
    int k[3];     // the chain's exercise step; N while the rule has not fired
    float Y;      // running: the product of the growth factors, dS/dS0 of EVERY scenario of this partner
    float Yu, Yd; // the bumped chains': Y at their exercise steps
    float Zx;     // base chain: the pair's Z at its step (this partner's W is +-sqrt(dt) Zx)
    int Ncx;      //             Nc
    float ZJx;    //             ZJ
};

// MODEL 0 GBM, 1/2/3/4 Heston scheme 0/1/2/3
template <int MODEL>
__device__ __forceinline__ float jg_grow(float s, float G)
{
    if constexpr (MODEL == 0) return s * G;
    else return heston_grow<MODEL - 1>(s, G);
}

// the count and the size normal of a step whose count word already passed thr[0]: jump_log2's own n and z_J
// (omc_jump_dev.h; the same compares and the same Philox block, so the compiler forms them once)
__device__ __forceinline__ void jump_draw(const JumpLaw& j, uint32_t w, uint64_t pair, int t, uint32_t stream, uint32_t k0,
                                          uint32_t k1, int& n, float& zj)
{
    n = 1;
#pragma unroll
    for (int k = 1; k < kJumpThr; ++k) n += w >= j.thr[k] ? 1 : 0;
    const U4 o = philox4x32_10((uint32_t)pair, (uint32_t)(pair >> 32), 0xC0000000u | (uint32_t)t, stream, k0, k1);
    float zs;
    box_muller(o.x, o.y, zj, zs);
}

// the decisions of one partner at step t, on spots already stepped
template <int PUT>
__device__ __forceinline__ void chains_decide(const JumpGreeksKArgs& a, JumpChains& ch, int t, const Fit& f, double invK,
                                              float Z, int Nc, float ZJ)
{
    const int N = a.g.n_steps;
    const bool last = t == N;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float s = ch.s[c];
        // (a step without a fit -- t = N among them -- has b0 = +inf: the rule does not fire; step N is the chain's when it
        // never has)
        const bool ex = exercises(pay_stored((double)s, a.K, invK, PUT), f) | (last & (ch.k[c] == N));
        ch.k[c] = ex ? t : ch.k[c];
        ch.sx[c] = ex ? s : ch.sx[c];
        if (c == 1) ch.Yu = ex ? ch.Y : ch.Yu;
        if (c == 2) ch.Yd = ex ? ch.Y : ch.Yd;
        if (c == 0) {
            ch.Zx = ex ? Z : ch.Zx;
            ch.Ncx = ex ? Nc : ch.Ncx;
            ch.ZJx = ex ? ZJ : ch.ZJx;
        }
    }
}

template <int MODEL, int PUT>
__global__ __launch_bounds__(kBlock) void jump_greeks_kernel(JumpGreeksKArgs a)
{
    extern __shared__ double sh_b[];  // [N+1][4]: b0, b1, b2 (b0 = +inf: no exercise at t)
    __shared__ double red[kNQ * kRedStride];
    const int tid = threadIdx.x;
    const int N = a.g.n_steps;
    fits_to_lds<false>(sh_b, nullptr, nullptr, a.betas, nullptr, N);
    const double K = a.K, invK = 1.0 / a.K;
    const int64_t p = (int64_t)blockIdx.x * kBlock + tid;
    const bool valid = p < a.g.P;

    JumpChains ca, cb;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ca.s[c] = cb.s[c] = c == 0 ? a.g.s_init : c == 1 ? a.s_up : a.s_dn;
        ca.sx[c] = cb.sx[c] = 0.0f;
        ca.k[c] = cb.k[c] = N;
    }
    ca.Zx = cb.Zx = ca.ZJx = cb.ZJx = 0.0f;
    ca.Y = cb.Y = 1.0f;
    ca.Yu = cb.Yu = ca.Yd = cb.Yd = 0.0f;
    ca.Ncx = cb.Ncx = 0;
    float va = a.g.v_init, vb = a.g.v_init;
    float Z = 0.0f, ZJ = 0.0f;  // the pair's running sums
    int Nc = 0;

    constexpr int SPB = MODEL == 0 ? 4 : 2;  // steps per Philox block of normals
    constexpr int NPC = 4 / SPB;             // blocks of normals per count block
    const int ncb = (N + 3) >> 2;
    const uint64_t pair = a.g.pair_offset + (uint64_t)(valid ? p : 0);
    const uint32_t thr0 = a.law.thr[0];
    int t = 0;
    for (int cblk = 0; cblk < ncb; ++cblk) {
        uint32_t w[4];  // the count words of steps 4 cblk + 1 .. 4 cblk + 4
        {
            const U4 o = philox4x32_10((uint32_t)pair, (uint32_t)(pair >> 32), 0x40000000u | (uint32_t)cblk, a.g.stream,
                                       a.g.k0, a.g.k1);
            w[0] = o.x >> 8; w[1] = o.y >> 8; w[2] = o.z >> 8; w[3] = o.w >> 8;
        }
#pragma unroll
        for (int h = 0; h < NPC; ++h) {
            if (t >= N) break;
            float z[4];
            normals4(pair, (uint32_t)(cblk * NPC + h), a.g.stream, a.g.k0, a.g.k1, z);
#pragma unroll
            for (int i = 0; i < SPB; ++i) {
                if (t >= N) break;
                ++t;
                const uint32_t wt = w[h * SPB + i];  // the step's word of the count block
                const bool jumps = wt >= thr0;
                float jl = 0.0f;
                if (__builtin_amdgcn_ballot_w64(jumps) != 0) {  // a lane of the wave jumps: everything a jump needs
                    if (jumps) {
                        jl = jump_log2(a.law, wt, pair, t, a.g.stream, a.g.k0, a.g.k1);
                        int n;
                        float zj;
                        jump_draw(a.law, wt, pair, t, a.g.stream, a.g.k0, a.g.k1, n, zj);
                        Nc += n;
                        ZJ = __builtin_fmaf(sqrtf((float)n), zj, ZJ);
                    }
                }
                float Ga, Gb;
                if constexpr (MODEL == 0) {
                    float e = __builtin_fmaf(a.g.b, z[i], a.g.a), ea = __builtin_fmaf(-a.g.b, z[i], a.g.a);
                    if (jumps) {
                        e += jl;
                        ea += jl;
                    }
                    Ga = fast_exp2(e);
                    Gb = fast_exp2(ea);
                    Z += z[i];
                } else {
                    heston_pair_factors<MODEL - 1>(a.g.hc, z[2 * i], z[2 * i + 1], va, vb, Ga, Gb);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    ca.s[c] = jg_grow<MODEL>(ca.s[c], Ga);
                    cb.s[c] = jg_grow<MODEL>(cb.s[c], Gb);
                }
                ca.Y = jg_grow<MODEL>(ca.Y, Ga);
                cb.Y = jg_grow<MODEL>(cb.Y, Gb);
                if constexpr (MODEL != 0) {
                    if (__builtin_amdgcn_ballot_w64(jumps) != 0) {
                        if (jumps) {
                            const float f = fast_exp2(jl);
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                ca.s[c] = ca.s[c] * f;
                                cb.s[c] = cb.s[c] * f;
                            }
                            ca.Y = ca.Y * f;
                            cb.Y = cb.Y * f;
                        }
                    }
                }
                const Fit f = fit_lds(sh_b, t);
                chains_decide<PUT>(a, ca, t, f, invK, Z, Nc, ZJ);
                chains_decide<PUT>(a, cb, t, f, invK, Z, Nc, ZJ);
            }
        }
    }

    // ---- the per-path terms, from the chains' own states alone
    double g0[kNQ], g1[kNQ], g2[kNQ], g3[kNQ];
#pragma unroll
    for (int q = 0; q < kNQ; ++q) g0[q] = g1[q] = g2[q] = g3[q] = 0.0;
    if (valid) {
        const double sign = PUT ? -1.0 : 1.0;
        const double T = a.T, dt = T / N, r = a.r, sqdt = sqrt(dt);
        const double ntot = (double)Nc;
        g2[6] = ntot;
        auto partner = [&](const JumpChains& ch, double eps) {
            // (no contraction: delta+ - delta- of two chains that stopped together is 0, not the rounding of one product)
#pragma clang fp contract(off)
            const int k = ch.k[0];
            const double imm = payoff_d(ch.sx[0], K, PUT);
            const double Dk = a.D[k - 1];
            const double cf = add_cash_flow(g0, imm, Dk, k < N);  // the pricing's cash-flow, bit for bit
            const double Dps = (imm > 0.0 ? sign : 0.0) * Dk * (double)ch.sx[0];  // D_k phi'(s) s
            const double delta = Dps / a.S0;
            g1[0] += delta;
            g1[1] += delta * delta;
            if constexpr (MODEL == 0) {
                const double tk = k * dt;
                const double W = eps * sqdt * (double)ch.Zx;
                const double vega = Dps * (-a.sigma * tk + W);
                const double epsl = -Dps * tk;
                const double rho = -(k - 1) * dt * cf - epsl;
                const double scoreT = cf * (ntot / T - a.lambda);
                const double theta = -(-r * (k - 1) / N * cf +
                                       Dps * ((a.rj - 0.5 * a.sigma * a.sigma) * k / N + a.sigma * W / (2.0 * T)) + scoreT);
                const double ltk = a.lambda * tk * a.kappa1;
                const double dmu = Dps * ((double)ch.Ncx - ltk);
                const double dsg = Dps * ((double)ch.ZJx - ltk * a.sigma_j);
                // (lambda = 0: the score is undefined; the caller reports NaN)
                const double dlam = Dps * (-a.kappa * tk) + (a.lambda > 0.0 ? cf * (ntot / a.lambda - T) : 0.0);
                g1[4] += vega;
                g1[5] += vega * vega;
                g1[6] += rho;
                g1[7] += rho * rho;
                g2[0] += theta;
                g2[1] += theta * theta;
                g2[4] += epsl;
                g2[5] += epsl * epsl;
                g3[0] += dlam;
                g3[1] += dlam * dlam;
                g3[2] += dmu;
                g3[3] += dmu * dmu;
                g3[4] += dsg;
                g3[5] += dsg * dsg;
                g3[6] -= scoreT;
                g3[7] += scoreT * scoreT;
            }
            double dlt[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int ke = ch.k[1 + s];
                const double ie = payoff_d(ch.sx[1 + s], K, PUT);
                const double De = a.D[ke - 1];
                g0[5 + s] += (ie > 0.0 ? ie : 0.0) * De;
                g2[2 + s] += ke < N ? 1.0 : 0.0;
                dlt[s] = (ie > 0.0 ? sign : 0.0) * De * (double)(s == 0 ? ch.Yu : ch.Yd);
            }
            const double gamma = (dlt[0] - dlt[1]) / (2.0 * a.h * a.S0);
            g1[2] += gamma;
            g1[3] += gamma * gamma;
        };
        partner(ca, 1.0);
        partner(cb, -1.0);
    }
    // four 8-quantity block reductions through one LDS patch; partials [kJumpGreeksQ][nwg]
    const size_t nwg = gridDim.x;
    double s = block_reduce8(g0, red);
    if (tid < 64 && (tid & 7) == 0) a.part[(size_t)(tid >> 3) * nwg + blockIdx.x] = s;
    __syncthreads();
    s = block_reduce8(g1, red);
    if (tid < 64 && (tid & 7) == 0) a.part[(size_t)(8 + (tid >> 3)) * nwg + blockIdx.x] = s;
    __syncthreads();
    s = block_reduce8(g2, red);
    if (tid < 64 && (tid & 7) == 0) a.part[(size_t)(16 + (tid >> 3)) * nwg + blockIdx.x] = s;
    __syncthreads();
    s = block_reduce8(g3, red);
    if (tid < 64 && (tid & 7) == 0) a.part[(size_t)(24 + (tid >> 3)) * nwg + blockIdx.x] = s;
}

// workgroup g adds quantities 8g .. 8g+7 over the sweep's partials (workgroup order fixed); slot 4 = the regression-set sizes
__global__ __launch_bounds__(kBlock) void jump_greeks_finalize_kernel(const double* __restrict__ part, int64_t nwg,
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

int64_t jump_greeks_blocks(int64_t n_paths)
{
    return (n_paths / 2 + kBlock - 1) / kBlock;
}

hipError_t jump_greeks(hipStream_t st, const JumpGreeksArgs& a, hipEvent_t ev_begin, hipEvent_t ev_end)
{
    const PathSpec& s = a.paths;
    const int64_t P = s.n_paths / 2;
    const int N = s.n_steps;
    if (P <= 0 || N < 1 || N > kMaxSteps) return hipErrorInvalidValue;
    JumpGreeksKArgs k{};
    k.g = make_path_args(s, P);
    k.law = a.law;
    k.s_up = (float)(s.S0 * (1.0 + a.h));
    k.s_dn = (float)(s.S0 * (1.0 - a.h));
    k.is_put = a.is_put ? 1 : 0;
    k.K = a.K; k.S0 = s.S0; k.r = a.r; k.T = s.T; k.h = a.h;
    k.sigma = s.sigma; k.rj = s.r;
    k.lambda = a.lambda; k.sigma_j = a.sigma_j; k.kappa = a.kappa; k.kappa1 = a.kappa + 1.0;
    k.D = a.D; k.betas = a.betas; k.part = a.part;
    const int64_t nwg = jump_greeks_blocks(s.n_paths);
    const size_t dyn = sizeof(double) * 4 * (size_t)(N + 1);
    if (ev_begin) (void)hipEventRecord(ev_begin, st);
    for_model(s.model, s.scheme, [&](auto model) {
        for_put(k.is_put, [&](auto put) {
            constexpr int MO = decltype(model)::value, PUT = decltype(put)::value;
            hipLaunchKernelGGL((jump_greeks_kernel<MO, PUT>), dim3((unsigned)nwg), dim3(kBlock), dyn, st, k);
        });
    });
    if (ev_end) (void)hipEventRecord(ev_end, st);
    hipLaunchKernelGGL(jump_greeks_finalize_kernel, dim3(4), dim3(kBlock), 0, st, a.part, nwg, a.gmom, N, a.result);
    return hipGetLastError();
}

}  // namespace omc
