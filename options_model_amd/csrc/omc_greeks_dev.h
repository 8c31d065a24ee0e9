// omc_greeks_dev.h -- the device bodies of the pathwise-Greeks sweep and of its finalize, shared by
// the single pricing's kernels (omc_greeks.hip) and the option chain's (omc_chain_greeks.hip).
//
// The chain's sweep runs the same body on a VIEW of the path matrix (omc_chain.h: the scheduled rows of a Bermudan entry,
// leading dimension `every` ld, Nv rows) with a step map: a chain that exercised at view row j exercised at fine step
//     t(j) = Nf - every (Nv - j),          "never" (j = Nv) -> Nf.
// The rows walked, the fits, the fold table and the valuation table D are the view's and are indexed by j; the three terms
// that name a TIME -- tk, (k - 1) dt and dt = T / Nf -- take the fine step and the fine N.  With every = 1 and Nf = Nv
// every integer, hence every double, is the plain body's.
#pragma once
#include "omc_greeks.h"
#include "omc_lsm_dev.h"

namespace omc {

// Where a workgroup of the body stands: column block blk() of nblk() -- columns [blk kBlock VEC, ..) of a.S, partials to
// a.part [kGreeksQ][nblk] at column blk -- and the step map.  The single pricing's: the grid is the column blocks, the rows
// walked are the steps (read where the body uses them, as its kernels always have).
struct GreeksGrid {
    static constexpr bool kView = false;  // (the body then names N and k themselves: no map stands between them and the terms)
    __device__ __forceinline__ unsigned blk() const { return blockIdx.x; }
    __device__ __forceinline__ size_t nblk() const { return gridDim.x; }
    __device__ __forceinline__ int fine_n(int N) const { return N; }
    __device__ __forceinline__ int step(int k, int) const { return k; }
};
// a chain entry's: the (column block, entry) pair comes from the launch's block order, the map is the view's (above)
struct GreeksViewGrid {
    static constexpr bool kView = true;
    int64_t blk_;
    size_t nblk_;
    int every, Nf;
    __device__ __forceinline__ int64_t blk() const { return blk_; }
    __device__ __forceinline__ size_t nblk() const { return nblk_; }
    __device__ __forceinline__ int fine_n(int) const { return Nf; }
    __device__ __forceinline__ int step(int j, int Nv) const { return Nf - every * (Nv - j); }
};

template <int VEC, bool FOLD, int PUT, class Grid>
__device__ __forceinline__ void greeks_body(const GreeksArgs& a, const Grid steps)
{
    extern __shared__ double sh_b[];  // [N+1][4]: b0, b1, b2 (b0 = +inf: no exercise at t), cK[t] when folded
    __shared__ double red[kNQ * kRedStride];
    const int tid = threadIdx.x;
    const int N = a.N;
    fits_to_lds<FOLD>(sh_b, nullptr, nullptr, a.betas, a.cK, N);
    const double K = a.K, invK = 1.0 / a.K;
    const double lup = 1.0 + a.h, ldn = 1.0 - a.h;
    const int64_t j = ((int64_t)steps.blk() * kBlock + tid) * VEC;
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
        const int nf = Grid::kView ? steps.fine_n(N) : N;
        const double S0 = a.S0, invS0 = 1.0 / a.S0, dt = a.T / nf, r = a.r, sig = a.sigma, T = a.T;
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
                    const int kf = Grid::kView ? steps.step(k, N) : k;  // the step's time
                    const double tk = kf * dt, lnr = log(s * invS0);
                    const double vega = Ds * (lnr - cvega * tk) / sig;
                    const double rho = -(kf - 1) * dt * cf + Ds * tk;
                    const double theta = -(-r * (kf - 1) * dt / T * cf + Ds * (lnr + ctheta * tk) / (2.0 * T));
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
    const size_t nblk = steps.nblk();
    double s = block_reduce8(g0, red);
    if (tid < 64 && (tid & 7) == 0) a.part[(size_t)(tid >> 3) * nblk + steps.blk()] = s;
    __syncthreads();
    s = block_reduce8(g1, red);
    if (tid < 64 && (tid & 7) == 0) a.part[(size_t)(8 + (tid >> 3)) * nblk + steps.blk()] = s;
    __syncthreads();
    s = block_reduce8(g2, red);
    if (tid < 64 && (tid & 7) == 0) a.part[(size_t)(16 + (tid >> 3)) * nblk + steps.blk()] = s;
}

// workgroup g adds quantities 8g .. 8g+7 over the sweep's partials (workgroup order fixed); slot 4 = the regression-set sizes
__device__ __forceinline__ void greeks_finalize_body(const double* __restrict__ part, int64_t nblk,
                                                     const double* __restrict__ gmom, int N, double* __restrict__ result,
                                                     int g)
{
    __shared__ double red[kNQ * kRedStride];
    const int tid = threadIdx.x;
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

}  // namespace omc
