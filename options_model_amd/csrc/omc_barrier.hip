// omc_barrier.hip -- knock-in / knock-out barrier options on the path matrix itself.
//
// One device body, barrier_paths_body<MODEL, STORE, MON, VEC>, launched as two kernels: STORE = true writes the ENCODED
// path matrix the unchanged two-pass LSM sweeps then price as an American option; STORE = false writes nothing.  Both
// reduce the European knock-out / knock-in sums of the same paths in the same order, so their sums are bit-equal.
//
// A lane owns VEC antithetic pairs.  Spots are those of gbm_paths_body / heston_pair_step<SCHEME> (omc_paths_dev.h):
// same Philox counters, same operations in the same order, hence the vanilla generator's bits wherever the option is
// live.  Per partner a knock state `hit` is kept (sticky):
//   discrete   at steps t = 1..N: down  (double)S_t <= H  <=>  S_t <= thr,  up  (double)S_t >= H  <=>  S_t >= thr,
//              thr the exact float32 threshold of barrier_threshold();
//   continuous (MON = 1, GBM only) also between grid points: a partner still live is hit at step t when u_t < p_t,
//              p_t = exp(-2 ln(S_{t-1}/H) ln(S_t/H) / (sigma^2 dt)), the Brownian-bridge crossing probability.  With
//              x = log2(S/H) tracked by the spot's own increment, x_t = x_{t-1} + (a +- b z_t), p_t = exp2((c x_{t-1}) x_t),
//              c = -2 ln 2 / (sigma^2 dt): one add, two multiplies and one v_exp_f32 per step and partner.  u_t is word
//              (t-1) & 3 of Philox block (pair, 0x80000000 | ((t-1) >> 2), stream) -- a counter domain no normal uses --
//              mapped by box_muller's u2 rule (w >> 8) 2^-24; both partners of a pair share it.
// Encoding (STORE): a knock-out is dead AT its hit step and after it, a knock-in is live FROM its hit step on (row 0 of a
// knock-in is dead).  A dead entry holds barrier_dead_spot(K) = itm_threshold(K, is_put): finite, payoff <= 0 and out of
// the money.  The full-storage two-pass sweeps never exercise it and it adds nothing to any sum:
//   lsm_pass1_body   u = fma(s, 1/K, -1) ~ 0 is finite, the in-the-money mask m = 0 zeroes it exactly (u * 0 = 0; an
//                    infinite or NaN dead value would give NaN here), and its terminal payoff pN = 0 (payoff_d <= 0);
//   lsm_pass2_body   imm = payoff_d <= 0 fails `imm > 0`, cont = fma(u, fma(u, b2, b1), b0) stays finite, and a path
//                    never exercised values max(payoff_d(S_N), 0) = 0 when S_N is dead.
// No grid-stride loop: a thread's 8 float64 sums are final after its pairs, then one block reduction per workgroup and a
// fixed-order finalize launch (as terminal_body + lsm_finalize): identical calls give identical bits.
#include "omc_barrier.h"
#include "omc_lsm_dev.h"
#include "omc_paths_dev.h"

namespace omc {

struct BarArgs {
    PathArgs g;  // S (null for STORE = false), ld, P = pairs, n_steps, s_init, a, b, v_init, hc, Philox key / stream / offset
    int is_put, knock_in;
    float sg, sthr;                 // hit iff sg * s <= sthr (down: 1, thr; up: -1, -thr)
    float dead;
    float x0, cbr;                  // continuous: log2(S0 / H), -2 ln 2 / (sigma^2 dt)
    double K, df;
    double* part;                   // [kBarrierQ][gridDim.x]
};

// VSTORE: one VEC-wide store (row starts and the partner half aligned to it).  A compile-time choice: with a run-time
// flag between the two forms the compiler merged them into scalar stores, and the generator took twice the time.
template <int VEC, bool VSTORE>
__device__ __forceinline__ void put_row(float* p, const float (&v)[VEC])
{
    if constexpr (VSTORE) {
        store_vec<VEC>(p, v);
    } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) p[k] = v[k];
    }
}

// MODEL 0 GBM, 1/2/3/4 Heston scheme 0/1/2/3; MON 0 discrete, 1 continuous (GBM only); VSTORE: VEC-wide stores
template <int MODEL, bool STORE, int MON, int VEC, bool VSTORE>
__device__ __forceinline__ void barrier_paths_body(const BarArgs& A)
{
    static_assert(MON == 0 || MODEL == 0, "continuous monitoring is GBM only");
    __shared__ double red[kNQ * kRedStride];
    const PathArgs& g = A.g;
    const int64_t P = g.P, ld = g.ld;
    const int64_t p0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * VEC;
    double acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0;
    if (p0 < P) {  // (P % VEC == 0: a thread's pairs all exist or none does)
        const float a = g.a, b = g.b, sg = A.sg, sthr = A.sthr, dead = A.dead, cbr = A.cbr;
        const bool ki = A.knock_in != 0;
        float s[VEC], sa[VEC], va[VEC], vb[VEC], x[VEC], xa[VEC];
        bool h[VEC], ha[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            s[v] = sa[v] = g.s_init;
            va[v] = vb[v] = g.v_init;
            x[v] = xa[v] = A.x0;
            h[v] = ha[v] = false;
        }
        float* row = STORE ? g.S + p0 : nullptr;
        if (STORE) {
            float e[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) e[v] = ki ? dead : g.s_init;
            put_row<VEC, VSTORE>(row, e);
            put_row<VEC, VSTORE>(row + P, e);
        }
        constexpr int SPB = MODEL == 0 ? 4 : 2;  // steps per Philox block of normals
        const int n_steps = g.n_steps;
        const int nblk = (n_steps + SPB - 1) / SPB;
        int t = 0;
        for (int blk = 0; blk < nblk; ++blk) {
            float z[VEC][4], u[VEC][4];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const uint64_t pair = g.pair_offset + (uint64_t)(p0 + v);
                normals4(pair, (uint32_t)blk, g.stream, g.k0, g.k1, z[v]);
                if (MON) {
                    const U4 o = philox4x32_10((uint32_t)pair, (uint32_t)(pair >> 32), 0x80000000u | (uint32_t)blk,
                                               g.stream, g.k0, g.k1);
                    u[v][0] = (float)(o.x >> 8) * 0x1p-24f;
                    u[v][1] = (float)(o.y >> 8) * 0x1p-24f;
                    u[v][2] = (float)(o.z >> 8) * 0x1p-24f;
                    u[v][3] = (float)(o.w >> 8) * 0x1p-24f;
                }
            }
#pragma unroll
            for (int i = 0; i < SPB; ++i) {
                if (++t > n_steps) break;
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    if constexpr (MODEL == 0) {
                        const float inc = __builtin_fmaf(b, z[v][i], a), inca = __builtin_fmaf(-b, z[v][i], a);
                        s[v] = s[v] * fast_exp2(inc);
                        sa[v] = sa[v] * fast_exp2(inca);
                        if (MON) {
                            const float xn = x[v] + inc, xna = xa[v] + inca;
                            h[v] |= u[v][i] < fast_exp2((cbr * x[v]) * xn);
                            ha[v] |= u[v][i] < fast_exp2((cbr * xa[v]) * xna);
                            x[v] = xn;
                            xa[v] = xna;
                        }
                    } else {
                        pair_step<MODEL>(g, z[v], i, s[v], va[v], sa[v], vb[v]);
                    }
                    h[v] |= sg * s[v] <= sthr;
                    ha[v] |= sg * sa[v] <= sthr;
                }
                if (STORE) {
                    row += ld;
                    float e[VEC], ea[VEC];
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        e[v] = (h[v] == ki) ? s[v] : dead;
                        ea[v] = (ha[v] == ki) ? sa[v] : dead;
                    }
                    put_row<VEC, VSTORE>(row, e);
                    put_row<VEC, VSTORE>(row + P, ea);
                }
            }
        }
        auto add = [&](float st, bool hit) {
            double p = payoff_d(st, A.K, A.is_put);
            p = p > 0.0 ? p * A.df : 0.0;
            const double po = hit ? 0.0 : p, pi = hit ? p : 0.0;
            acc[0] += po;
            acc[1] += po * po;
            acc[2] += pi;
            acc[3] += pi * pi;
            acc[4] += hit ? 1.0 : 0.0;
        };
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            add(s[v], h[v]);
            add(sa[v], ha[v]);
        }
    }
    const double r = block_reduce8(acc, red);
    if (threadIdx.x < 64 && (threadIdx.x & 7) == 0) A.part[(size_t)(threadIdx.x >> 3) * gridDim.x + blockIdx.x] = r;
}

template <int MODEL, bool STORE, int MON, int VEC, bool VSTORE>
__global__ __launch_bounds__(kBlock) void barrier_paths_kernel(BarArgs a)
{
    barrier_paths_body<MODEL, STORE, MON, VEC, VSTORE>(a);
}

// part [kBarrierQ][nblk] -> result [kBarrierQ], one workgroup, fixed order
__global__ __launch_bounds__(kBlock) void barrier_finalize_kernel(const double* __restrict__ part, int64_t nblk,
                                                                  double* __restrict__ result)
{
    __shared__ double red[kNQ * kRedStride];
    double acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0;
    for (int64_t i = threadIdx.x; i < nblk; i += kBlock) {
#pragma unroll
        for (int q = 0; q < kBarrierQ; ++q) acc[q] += part[(size_t)q * nblk + i];
    }
    const double s = block_reduce8(acc, red);
    if (threadIdx.x < 64 && (threadIdx.x & 7) == 0) result[threadIdx.x >> 3] = s;
}

// ------------------------------------------------------------------ host side
static float next_float_h(float f, bool up)
{
    return std::nextafter(f, up ? INFINITY : -INFINITY);
}

float barrier_dead_spot(double K, int is_put)
{
    // itm_threshold (omc_lsm_dev.h) on the host
    const float Kf = (float)K;
    if (is_put) return (double)Kf < K ? next_float_h(Kf, true) : Kf;
    return (double)Kf > K ? next_float_h(Kf, false) : Kf;
}

float barrier_threshold(double H, int up)
{
    const float Hf = (float)H;
    if (up) return (double)Hf < H ? next_float_h(Hf, true) : Hf;
    return (double)Hf > H ? next_float_h(Hf, false) : Hf;
}

int barrier_vec(const BarrierGen& a)
{
    return ((a.paths.n_paths / 2) % 4) == 0 ? 4 : 1;  // from the geometry only: both kernels reduce in the same order
}

int64_t barrier_blocks(const BarrierGen& a)
{
    const int64_t per = (int64_t)kBlock * barrier_vec(a);
    const int64_t P = a.paths.n_paths / 2;
    return P > 0 ? (P + per - 1) / per : 1;
}

hipError_t launch_barrier_paths(hipStream_t st, const BarrierGen& a)
{
    const PathSpec& s = a.paths;
    const int vec = barrier_vec(a);
    const int64_t nblk = barrier_blocks(a);
    BarArgs A{};
    A.g = make_path_args(s, s.n_paths / 2);
    A.is_put = a.is_put; A.knock_in = a.knock_in;
    const bool vstore = s.S && vec > 1 && rows_aligned(vec, A.g.P, s.S, s.ld);
    const float thr = barrier_threshold(a.H, a.up);
    A.sg = a.up ? -1.0f : 1.0f;
    A.sthr = a.up ? -thr : thr;
    A.dead = barrier_dead_spot(a.K, a.is_put);
    A.x0 = (float)std::log2((double)(float)s.S0 / a.H);
    A.cbr = s.model == 0 ? (float)(-2.0 * 0.69314718055994530942 / (s.sigma * s.sigma * (s.T / s.n_steps))) : 0.0f;
    A.K = a.K; A.df = exp(-s.r * s.T); A.part = a.part;
    const dim3 grid((unsigned)nblk), block(kBlock);
    for_flag(s.S != nullptr, [&](auto store) {
        for_int<1, 0>(s.model == 0 && a.continuous ? 1 : 0, [&](auto mon) {
            for_model(s.model, s.scheme, [&](auto model) {
                constexpr int MO = decltype(model)::value, MN = decltype(mon)::value;
                constexpr bool STO = decltype(store)::value;
                if constexpr (MN == 0 || MO == 0) {  // (continuous monitoring is GBM only)
                    if (STO && vec == 4 && vstore)  // (VEC-wide stores only where there are stores)
                        hipLaunchKernelGGL((barrier_paths_kernel<MO, STO, MN, 4, STO>), grid, block, 0, st, A);
                    else if (vec == 4) hipLaunchKernelGGL((barrier_paths_kernel<MO, STO, MN, 4, false>), grid, block, 0, st, A);
                    else hipLaunchKernelGGL((barrier_paths_kernel<MO, STO, MN, 1, false>), grid, block, 0, st, A);
                }
            });
        });
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(barrier_finalize_kernel, dim3(1), dim3(kBlock), 0, st, (const double*)a.part, nblk, a.result);
    return hipGetLastError();
}

}  // namespace omc
