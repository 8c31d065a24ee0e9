// omc_greeks.hip -- pathwise Greeks of the two-pass (v3) polynomial-LSM estimator with the exercise policy FROZEN
// (DESIGN.md section 10).  One extra sweep over the path matrix the pricing already holds.
//
// Every stored spot of every model here is proportional to S0, so the scenario "S0 bumped by a factor lambda" is the
// stored path times lambda: no new paths.  Per path the sweep follows three CHAINS -- lambda = 1 (the base pricing,
// with pass 2's very expressions), 1 + h and 1 - h -- each deciding with the same frozen fits on spot lambda s_t and
// remembering its own (exercise spot, exercise step).  On folded storage (omc_lsm_dev.h) the partner of every stored
// column has three chains as well: six per column.  All Greek terms are formed once, after the sweep, from those pairs:
//   delta  D_k phi'(s) s / S0                          vega  D_k phi'(s) s (ln(s/S0) - (r + sigma^2/2) k dt) / sigma
//   rho    -(k-1) dt cf + D_k phi'(s) s k dt           theta -[-r (k-1) dt / T cf + D_k phi'(s) s (ln(s/S0) + (r - sigma^2/2) k dt) / 2T]
//   gamma  (delta+ - delta-) / (2 h S0), delta+- = D_k+- phi'(lambda+- s_k+-) s_k+- / S0
// with D_k = D[k-1] (valued at t = dt, as the pricing) and phi' = -1{imm > 0} (put) / +1{imm > 0} (call).
//
// One thread owns VEC columns and walks them backward until every chain has exercised; rows arrive in batches with
// the next batch requested before the current one is decided (walk_rows, as the folded pass 2).  Grid = one thread per VEC columns
// (no grid-stride loop: the 20 sums are live only after the sweep), per-workgroup partials in a fixed order, then one
// finalize launch: two identical calls return identical bits.
#include "omc_greeks.h"
#include "omc_lsm_dev.h"

namespace omc {

template <int VEC, bool FOLD, int PUT>
__device__ __forceinline__ void greeks_body(const GreeksArgs& a)
{
    extern __shared__ double sh_b[];  // [N+1][4]: b0, b1, b2 (b0 = +inf: no exercise at t), cK[t] when folded
    __shared__ double red[kNQ * kRedStride];
    const int tid = threadIdx.x;
    const int N = a.N;
    fits_to_lds<FOLD>(sh_b, nullptr, nullptr, a.betas, a.cK, N);
    const double K = a.K, invK = 1.0 / a.K;
    const double lup = 1.0 + a.h, ldn = 1.0 - a.h;
    const int64_t j = ((int64_t)blockIdx.x * kBlock + tid) * VEC;
    const bool valid = j < a.cols;  // (cols % VEC == 0: a thread's columns all exist or none does)
    const float* col = a.S + (valid ? j : 0);

    // chain c of column v: 0 base, 1 up, 2 down (the stored path); 3, 4, 5 the same for its partner (folded)
    constexpr int C = FOLD ? 6 : 3;
    float sx[C][VEC];    // the STORED spot at the chain's exercise step (a partner's own spot is rebuilt from it)
    int32_t tx[C][VEC];  // its exercise step, N while it has not exercised
    {
        float sn[VEC];
        loadf<VEC>(col + (int64_t)N * a.ld, sn);
#pragma unroll
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                sx[c][v] = sn[v];
                tx[c][v] = valid ? N : 0;  // a lane without columns is never live
            }
        }
    }
    auto decide = [&](const float (&row)[VEC], int t) {
        const Fit f = fit_lds(sh_b, t);
        auto chain = [&](int c, int v, const PayU& p) {
            const bool ex = (tx[c][v] == N) & exercises(p, f);
            sx[c][v] = ex ? row[v] : sx[c][v];
            tx[c][v] = ex ? t : tx[c][v];
        };
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            // the bumped chains decide on spot lambda * spot, in double
            const double sd = (double)row[v];
            chain(0, v, pay_stored(sd, K, invK, PUT));
            chain(1, v, pay_stored(lup * sd, K, invK, PUT));
            chain(2, v, pay_stored(ldn * sd, K, invK, PUT));
            if constexpr (FOLD) {
                const PayU pb = pay_partner(sh_b[4 * t + 3], row[v], K, PUT);
                chain(3, v, pb);
                const double sb = K * (1.0 + pb.u);
                chain(4, v, pay_stored(lup * sb, K, invK, PUT));
                chain(5, v, pay_stored(ldn * sb, K, invK, PUT));
            }
        }
    };
    auto live = [&]() {
        bool l = false;
#pragma unroll
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) l |= tx[c][v] == N;
        }
        return l;
    };
    walk_rows<VEC, false>(col, a.ld, N, decide, live);

    // ---- the per-path terms, from the (spot, step) pairs alone
    double g0[kNQ], g1[kNQ], g2[kNQ];
#pragma unroll
    for (int q = 0; q < kNQ; ++q) g0[q] = g1[q] = g2[q] = 0.0;
    if (valid) {
        const double sign = PUT ? -1.0 : 1.0;
        const double S0 = a.S0, invS0 = 1.0 / a.S0, dt = a.T / N, r = a.r, sig = a.sigma, T = a.T;
        const double cvega = r + 0.5 * sig * sig, ctheta = r - 0.5 * sig * sig;
        // the spot of chain c at its exercise step: the stored one, or the partner's K (1 + u')
        auto spot = [&](int c, int v) {
            if (FOLD && c >= 3) return K * (1.0 + fold_u(sh_b[4 * tx[c][v] + 3], sx[c][v]));
            return (double)sx[c][v];
        };
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
#pragma unroll
            for (int p = 0; p < (FOLD ? 2 : 1); ++p) {
                const int c = 3 * p;
                const int k = tx[c][v];
                double s, imm;
                if (p == 0) {
                    s = (double)sx[c][v];
                    imm = payoff_d(sx[c][v], K, PUT);
                } else {
                    const PayU pb = pay_partner(sh_b[4 * k + 3], sx[c][v], K, PUT);
                    imm = pb.imm;
                    s = K * (1.0 + pb.u);
                }
                const double Dk = a.D[k - 1];
                const double cf = add_cash_flow(g0, imm, Dk, k < N);  // the pricing's cash-flow, bit for bit
                const double Ds = (imm > 0.0 ? sign : 0.0) * Dk * s;  // D_k phi'(s) s
                const double delta = Ds * invS0;
                g1[0] += delta;
                g1[1] += delta * delta;
                if (a.gbm) {
                    const double tk = k * dt, lnr = log(s * invS0);
                    const double vega = Ds * (lnr - cvega * tk) / sig;
                    const double rho = -(k - 1) * dt * cf + Ds * tk;
                    const double theta = -(-r * (k - 1) * dt / T * cf + Ds * (lnr + ctheta * tk) / (2.0 * T));
                    g1[4] += vega;
                    g1[5] += vega * vega;
                    g1[6] += rho;
                    g1[7] += rho * rho;
                    g2[0] += theta;
                    g2[1] += theta * theta;
                }
                double dlt[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int ce = c + 1 + e;
                    const int ke = tx[ce][v];
                    const double se = spot(ce, v), ls = (e == 0 ? lup : ldn) * se;
                    const double ie = PUT ? K - ls : ls - K;
                    const double De = a.D[ke - 1];
                    g0[5 + e] += (ie > 0.0 ? ie : 0.0) * De;
                    g2[2 + e] += ke < N ? 1.0 : 0.0;
                    dlt[e] = (ie > 0.0 ? sign : 0.0) * De * se * invS0;
                }
                const double gamma = (dlt[0] - dlt[1]) / (2.0 * a.h * S0);
                g1[2] += gamma;
                g1[3] += gamma * gamma;
            }
        }
    }
    // three 8-quantity block reductions through one LDS patch; partials [kGreeksQ][nblk]
    const size_t nblk = gridDim.x;
    double s = block_reduce8(g0, red);
    if (tid < 64 && (tid & 7) == 0) a.part[(size_t)(tid >> 3) * nblk + blockIdx.x] = s;
    __syncthreads();
    s = block_reduce8(g1, red);
    if (tid < 64 && (tid & 7) == 0) a.part[(size_t)(8 + (tid >> 3)) * nblk + blockIdx.x] = s;
    __syncthreads();
    s = block_reduce8(g2, red);
    if (tid < 64 && (tid & 7) == 0) a.part[(size_t)(16 + (tid >> 3)) * nblk + blockIdx.x] = s;
}

template <int VEC, bool FOLD, int PUT>
__global__ __launch_bounds__(kBlock) void lsm_greeks_kernel(GreeksArgs a)
{
    greeks_body<VEC, FOLD, PUT>(a);
}

// workgroup g adds quantities 8g .. 8g+7 over the sweep's partials (workgroup order fixed); slot 4 = the regression-set sizes
__global__ __launch_bounds__(kBlock) void lsm_greeks_finalize_kernel(const double* __restrict__ part, int64_t nblk,
                                                                     const double* __restrict__ gmom, int N,
                                                                     double* __restrict__ result)
{
    __shared__ double red[kNQ * kRedStride];
    const int tid = threadIdx.x, g = blockIdx.x;
    double acc[kNQ];
#pragma unroll
    for (int q = 0; q < kNQ; ++q) acc[q] = 0.0;
    for (int64_t i = tid; i < nblk; i += kBlock) {
#pragma unroll
        for (int q = 0; q < kNQ; ++q) acc[q] += part[(size_t)(8 * g + q) * nblk + i];
    }
    if (g == 0 && gmom) {
        for (int t = 1 + tid; t < N; t += kBlock) acc[4] += gmom[(size_t)t * 8];
    }
    const double s = block_reduce8(acc, red);
    if (tid < 64 && (tid & 7) == 0) result[8 * g + (tid >> 3)] = s;
}

int greeks_vec(const GreeksArgs& a)
{
    return rows_aligned(2, a.cols, a.S, a.ld) ? 2 : 1;
}

int64_t greeks_blocks(const GreeksArgs& a)
{
    const int64_t per = (int64_t)kBlock * greeks_vec(a);
    return (a.cols + per - 1) / per;
}

hipError_t lsm_greeks(hipStream_t st, const GreeksArgs& a, hipEvent_t ev_begin, hipEvent_t ev_end)
{
    const int64_t nblk = greeks_blocks(a);
    const size_t dyn = sizeof(double) * 4 * (size_t)(a.N + 1);
    if (ev_begin) (void)hipEventRecord(ev_begin, st);
    for_int<2, 1>(greeks_vec(a), [&](auto vec) {
        for_flag(a.cK != nullptr, [&](auto fold) {
            for_put(a.is_put, [&](auto put) {
                constexpr int VEC = decltype(vec)::value, PUT = decltype(put)::value;
                hipLaunchKernelGGL((lsm_greeks_kernel<VEC, decltype(fold)::value, PUT>), dim3((unsigned)nblk), dim3(kBlock), dyn,
                                   st, a);
            });
        });
    });
    if (ev_end) (void)hipEventRecord(ev_end, st);
    hipLaunchKernelGGL(lsm_greeks_finalize_kernel, dim3(3), dim3(kBlock), 0, st, a.part, nblk, a.gmom, a.N, a.result);
    return hipGetLastError();
}

}  // namespace omc
