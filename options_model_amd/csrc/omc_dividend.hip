// omc_dividend.hip -- path generator for a stock that pays discrete dividends.
//
// dividend_paths_kernel<MODEL, VEC> writes the full-storage path matrix the unchanged two-pass LSM sweeps then price.
// A lane owns VEC antithetic pairs.  Spots are those of gbm_paths_body / heston_pair_step<SCHEME> (omc_paths_dev.h):
// same Philox counters, same operations, hence the vanilla generator's bits up to the first dividend step.  On a
// dividend step k, after the model's own step, both partners become
//     s = fmaxf(fmaf(s, mul_k, -cash_k), 0)                (the Heston variance is untouched)
// so row k holds the EX-dividend spot.  (mul_k, cash_k) compose every dividend of the step on the host in float64
// (omc_dividend_schedule).
//
// The dividend steps come as a short table sorted by step and closed by an entry no step reaches.  A wave keeps the
// NEXT entry in scalar registers: the per-step test is one scalar compare of the loop counter with it, indexed by t
// only, and a step without a dividend executes no fma / max and reads nothing.  The table is read by uniform loads,
// one 16-byte entry per dividend step.  No grid-stride loop; every write is a VEC-wide vector store.
#include "omc_dividend.h"
#include "omc_paths_dev.h"

namespace omc {

HestonC make_heston(double r, double T, int n_steps, double kappa, double theta, double xi, double rho);

// MODEL 0 GBM, 1/2/3 Heston scheme 0/1/2.  VEC-wide stores: the launcher picks a VEC every row start is aligned to.
template <int MODEL, int VEC>
__global__ __launch_bounds__(kBlock) void dividend_paths_kernel(PathArgs g, const DivEntry* __restrict__ tab)
{
    const int64_t P = g.P, ld = g.ld;
    const int64_t p0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * VEC;
    if (p0 >= P) return;  // (P % VEC == 0: a thread's pairs all exist or none does)
    const float a = g.a, b = g.b;
    float s[VEC], sa[VEC], va[VEC], vb[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        s[v] = sa[v] = g.s_init;
        va[v] = vb[v] = g.v_init;
    }
    float* row = g.S + p0;
    store_vec<VEC>(row, s);
    store_vec<VEC>(row + P, sa);
    constexpr int SPB = MODEL == 0 ? 4 : 2;  // steps per Philox block of normals
    const int n_steps = g.n_steps;
    const int nblk = (n_steps + SPB - 1) / SPB;
    DivEntry e = tab[0];  // the next dividend step: the same for every lane
    int next = 1;
    int t = 0;
    for (int blk = 0; blk < nblk; ++blk) {
        float z[VEC][4];
#pragma unroll
        for (int v = 0; v < VEC; ++v) normals4(g.pair_offset + (uint64_t)(p0 + v), (uint32_t)blk, g.stream, g.k0, g.k1, z[v]);
#pragma unroll
        for (int i = 0; i < SPB; ++i) {
            if (++t > n_steps) break;
            row += ld;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if constexpr (MODEL == 0) {
                    s[v] = s[v] * fast_exp2(__builtin_fmaf(b, z[v][i], a));
                    sa[v] = sa[v] * fast_exp2(__builtin_fmaf(-b, z[v][i], a));
                } else {
                    heston_pair_step<MODEL - 1>(g.hc, z[v][2 * i], z[v][2 * i + 1], s[v], va[v], sa[v], vb[v]);
                }
            }
            if (t == e.step) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    s[v] = __builtin_fmaxf(__builtin_fmaf(s[v], e.mul, -e.cash), 0.0f);
                    sa[v] = __builtin_fmaxf(__builtin_fmaf(sa[v], e.mul, -e.cash), 0.0f);
                }
                e = tab[next++];
            }
            store_vec<VEC>(row, s);
            store_vec<VEC>(row + P, sa);
        }
    }
}

hipError_t launch_dividend_paths(hipStream_t st, const DividendGen& a)
{
    const double dt = a.T / a.n_steps, L2E = 1.4426950408889634074;
    const int64_t P = a.n_paths / 2;
    if (P <= 0) return hipSuccess;
    int vec = a.vec_hint > 0 ? a.vec_hint : 4;
    // VEC-wide stores need every row start and the antithetic half aligned (as launch_gbm_paths)
    while (vec > 1 && !((P % vec) == 0 && (a.ld % vec) == 0 && ((uintptr_t)a.S % (4 * vec)) == 0)) vec >>= 1;
    PathArgs g{};
    g.S = a.S; g.ld = a.ld; g.P = P; g.n_steps = a.n_steps;
    g.s_init = (float)a.S0; g.v_init = (float)a.v0;
    g.a = (float)((a.r - 0.5 * a.sigma * a.sigma) * dt * L2E);
    g.b = (float)(a.sigma * sqrt(dt) * L2E);
    if (a.model != 0) g.hc = make_heston(a.r, a.T, a.n_steps, a.kappa, a.theta, a.xi, a.rho);
    g.k0 = (uint32_t)a.seed; g.k1 = (uint32_t)(a.seed >> 32); g.stream = a.stream; g.pair_offset = a.pair_offset;
    auto go = [&](auto model) {
        constexpr int MO = decltype(model)::value;
        const dim3 block(kBlock);
        auto grid = [&](int v) { return dim3((unsigned)((P / v + kBlock - 1) / kBlock)); };
        if (vec == 4) hipLaunchKernelGGL((dividend_paths_kernel<MO, 4>), grid(4), block, 0, st, g, a.tab);
        else if (vec == 2) hipLaunchKernelGGL((dividend_paths_kernel<MO, 2>), grid(2), block, 0, st, g, a.tab);
        else hipLaunchKernelGGL((dividend_paths_kernel<MO, 1>), grid(1), block, 0, st, g, a.tab);
    };
    using std::integral_constant;
    if (a.model == 0) go(integral_constant<int, 0>{});
    else if (a.scheme == 0) go(integral_constant<int, 1>{});
    else if (a.scheme == 1) go(integral_constant<int, 2>{});
    else go(integral_constant<int, 3>{});
    return hipGetLastError();
}

}  // namespace omc
