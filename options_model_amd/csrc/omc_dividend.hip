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

// MODEL 0 GBM, 1/2/3/4 Heston scheme 0/1/2/3.  VEC-wide stores: the launcher picks a VEC every row start is aligned to.
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
    const PathSpec& s = a.paths;
    const int64_t P = s.n_paths / 2;
    if (P <= 0) return hipSuccess;
    const PathArgs g = make_path_args(s, P);
    const int width = store_vec_width(s.vec_hint, P, s.S, s.ld);  // (so P % VEC == 0 and every store is VEC wide)
    for_model(s.model, s.scheme, [&](auto model) {
        for_vec(width, [&](auto vec) {
            constexpr int MO = decltype(model)::value, V = decltype(vec)::value;
            hipLaunchKernelGGL((dividend_paths_kernel<MO, V>), dim3((unsigned)((P / V + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                               st, g, a.tab);
        });
    });
    return hipGetLastError();
}

}  // namespace omc
