// omc_basket.hip -- path generator of the multi-asset options: basket (arithmetic / geometric), best-of and worst-of,
// DESIGN.md section 16; and the running averages of the basket value, the Asian kinds of section 23.
//
// basket_paths_kernel<D, VEC, KEEP> writes the full-storage matrix of the INDEX X_t of D correlated GBM assets, which the
// unchanged two-pass LSM sweeps then price.  A lane owns VEC antithetic pairs for all steps and holds the 2 D VEC asset
// spots (and the 2 VEC geometric states) in registers; only the index leaves, and with KEEP the asset rows too.  Asset k
// draws the vanilla generator's normals at the pair index pair + (k << 40) (include/omc.h): one Philox block per asset
// per pair per four steps.  The correlated normals y_i = sum_{k <= i} Lf[i][k] z_k are accumulated while the z_k are
// generated, k ascending -- the order the header fixes -- so a lane never holds more than one asset's raw normals.  The
// step of an asset is gbm_paths_body's (omc_paths_dev.h): same counters, same operations.  The correlation and the index
// rule are omc_basket_dev.h's, which the bound kernels (omc_basket_bounds.hip) use too.
//
// The per-asset constants, the packed Cholesky factor and the kind come by value in the argument block: scalar
// registers, no table in memory.  D is a template parameter so that every loop over assets unrolls and every index of
// the constants is a compile-time one; the kind is wave-uniform and switched on where the index is formed.  No
// grid-stride loop, no LDS; every write is a VEC-wide vector store.
//
// The Asian kinds (include/omc.h) form the index from a running state per partner -- c += B_t, X_t = c * (1.0f / t), or
// l += log2(B_t), X_t = exp2(l * (1.0f / t)) -- with B_t the arithmetic basket value of the step: one more register per
// partner, no more memory traffic, the same launch shape.  The bound kernels' inner paths start from that state, so a
// caller inside the library may have it stored beside the asset rows (BasketGen::state).
#include "omc_basket.h"
#include "omc_basket_dev.h"
#include "omc_paths_dev.h"

namespace omc {

struct BasketArgs {
    float* S;       // index matrix [N+1][ld]
    float* A;       // asset matrices [D][N+1][lda] (KEEP only)
    float* C;       // running state of the Asian kinds [N+1][lda], or null (KEEP only)
    int64_t ld, lda, P;
    int n_steps;
    uint32_t k0, k1, stream;
    uint64_t pair_offset;
};

// ASIAN: the two running-average kinds (OMC_BASKET_ASIAN_*), an instantiation of their own so that the kernels of kinds
// 0 .. 3 keep their instruction streams.  The running state -- c_t, the float32 sum of the basket values B_1 .. B_t, or
// l_t, the sum of their log2 -- is one more register per partner; with g.C it is stored beside the asset rows.
template <int D, int VEC, bool KEEP, bool ASIAN = false>
__global__ __launch_bounds__(kBlock) void basket_paths_kernel(BasketArgs g, BasketLaw c)
{
    const int64_t P = g.P, ld = g.ld;
    const int64_t p0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * VEC;
    if (p0 >= P) return;  // (P % VEC == 0: a thread's pairs all exist or none does)
    const int kind = c.kind;
    const bool geo = kind == OMC_BASKET_GEOMETRIC;
    float s[VEC][D], sa[VEC][D], gs[VEC], ga[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
#pragma unroll
        for (int k = 0; k < D; ++k) s[v][k] = sa[v][k] = c.s0[k];
        gs[v] = ga[v] = c.g0;
    }
    float* row = g.S + p0;
    float* arow = KEEP ? g.A + p0 : nullptr;
    const int64_t astride = KEEP ? (int64_t)(g.n_steps + 1) * g.lda : 0;  // one asset's matrix
    [[maybe_unused]] float cs[VEC], ca[VEC];  // ASIAN: the running state of either partner
    [[maybe_unused]] float* crow = nullptr;
    [[maybe_unused]] int t = 0;
    if constexpr (ASIAN) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) cs[v] = ca[v] = 0.0f;
        if constexpr (KEEP) crow = g.C ? g.C + p0 : nullptr;
    }

    auto store_rows = [&]() {
        float x[VEC], xa[VEC];
        if constexpr (ASIAN) {
            // B_t by the arithmetic rule; row 0 is B_0 and leaves the state at 0.  inv_t is wave-uniform
            const float inv_t = __fdiv_rn(1.0f, (float)(t > 0 ? t : 1));
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float B = basket_index<OMC_BASKET_ARITHMETIC, D>(c, s[v]);
                const float Ba = basket_index<OMC_BASKET_ARITHMETIC, D>(c, sa[v]);
                if (t == 0) {
                    x[v] = B;
                    xa[v] = Ba;
                } else if (kind == OMC_BASKET_ASIAN_ARITHMETIC) {
                    cs[v] = asian_add(cs[v], B);
                    ca[v] = asian_add(ca[v], Ba);
                    x[v] = cs[v] * inv_t;
                    xa[v] = ca[v] * inv_t;
                } else {
                    cs[v] = cs[v] + __builtin_amdgcn_logf(B);
                    ca[v] = ca[v] + __builtin_amdgcn_logf(Ba);
                    x[v] = fast_exp2(cs[v] * inv_t);
                    xa[v] = fast_exp2(ca[v] * inv_t);
                }
            }
            if constexpr (KEEP) {
                if (crow) {
                    store_vec<VEC>(crow, cs);
                    store_vec<VEC>(crow + P, ca);
                }
            }
        } else if (geo) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                x[v] = gs[v];
                xa[v] = ga[v];
            }
        } else if (kind == OMC_BASKET_ARITHMETIC) {  // (the kind is wave-uniform: one scalar branch per row, not per pair)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                x[v] = basket_index<OMC_BASKET_ARITHMETIC, D>(c, s[v]);
                xa[v] = basket_index<OMC_BASKET_ARITHMETIC, D>(c, sa[v]);
            }
        } else if (kind == OMC_BASKET_BEST_OF) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                x[v] = basket_index<OMC_BASKET_BEST_OF, D>(c, s[v]);
                xa[v] = basket_index<OMC_BASKET_BEST_OF, D>(c, sa[v]);
            }
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                x[v] = basket_index<OMC_BASKET_WORST_OF, D>(c, s[v]);
                xa[v] = basket_index<OMC_BASKET_WORST_OF, D>(c, sa[v]);
            }
        }
        store_vec<VEC>(row, x);
        store_vec<VEC>(row + P, xa);
        if constexpr (KEEP) {
#pragma unroll
            for (int k = 0; k < D; ++k) {
                float t[VEC], ta[VEC];
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    t[v] = s[v][k];
                    ta[v] = sa[v][k];
                }
                store_vec<VEC>(arow + k * astride, t);
                store_vec<VEC>(arow + k * astride + P, ta);
            }
        }
    };
    store_rows();

    const int n_steps = g.n_steps;
    const int nblk = (n_steps + 3) >> 2;
    for (int blk = 0; blk < nblk; ++blk) {
        float y[VEC][D][4];  // the correlated normals of the block's four steps
#pragma unroll
        for (int k = 0; k < D; ++k) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                float z[4];
                normals4(g.pair_offset + (uint64_t)(p0 + v) + ((uint64_t)k << 40), (uint32_t)blk, g.stream, g.k0, g.k1, z);
                basket_correlate<D>(c, k, z, y[v]);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (++t > n_steps) break;
            row += ld;
            if constexpr (KEEP) arow += g.lda;
            if constexpr (ASIAN && KEEP) crow = crow ? crow + g.lda : nullptr;
            if (geo) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    float E = 0.0f, Ea = 0.0f;
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        const float e = __builtin_fmaf(c.b[k], y[v][k][j], c.a[k]);
                        const float ea = __builtin_fmaf(-c.b[k], y[v][k][j], c.a[k]);
                        s[v][k] = s[v][k] * fast_exp2(e);
                        sa[v][k] = sa[v][k] * fast_exp2(ea);
                        E = k == 0 ? c.w[0] * e : __builtin_fmaf(c.w[k], e, E);
                        Ea = k == 0 ? c.w[0] * ea : __builtin_fmaf(c.w[k], ea, Ea);
                    }
                    gs[v] = gs[v] * fast_exp2(E);
                    ga[v] = ga[v] * fast_exp2(Ea);
                }
            } else {
                // basket_step's arithmetic (omc_basket_dev.h), which this loop must match: it is restated here, beside the
                // geometric branch, because through the helper the D >= 2 kernels come out with another schedule
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        s[v][k] = s[v][k] * fast_exp2(__builtin_fmaf(c.b[k], y[v][k][j], c.a[k]));
                        sa[v][k] = sa[v][k] * fast_exp2(__builtin_fmaf(-c.b[k], y[v][k][j], c.a[k]));
                    }
                }
            }
            store_rows();
        }
    }
}

template <int D, int VEC>
static void launch_basket(hipStream_t st, const BasketArgs& g, const BasketLaw& law, bool keep)
{
    const dim3 block(kBlock), grid((unsigned)((g.P / VEC + kBlock - 1) / kBlock));
    if (basket_kind_is_asian(law.kind)) {
        if (keep) hipLaunchKernelGGL((basket_paths_kernel<D, VEC, true, true>), grid, block, 0, st, g, law);
        else hipLaunchKernelGGL((basket_paths_kernel<D, VEC, false, true>), grid, block, 0, st, g, law);
        return;
    }
    if (keep) hipLaunchKernelGGL((basket_paths_kernel<D, VEC, true>), grid, block, 0, st, g, law);
    else hipLaunchKernelGGL((basket_paths_kernel<D, VEC, false>), grid, block, 0, st, g, law);
}

template <int D>
static void launch_basket_d(hipStream_t st, const BasketArgs& g, const BasketLaw& law, bool keep, int vec)
{
    constexpr int CAP = basket_vec_cap(D);
    if constexpr (CAP >= 4) {
        if (vec == 4) return launch_basket<D, 4>(st, g, law, keep);
    }
    if constexpr (CAP >= 2) {
        if (vec >= 2) return launch_basket<D, 2>(st, g, law, keep);
    }
    launch_basket<D, 1>(st, g, law, keep);
}

hipError_t launch_basket_paths(hipStream_t st, const BasketGen& a)
{
    const PathSpec& s = a.paths;
    const int64_t P = s.n_paths / 2;
    if (P <= 0) return hipSuccess;
    if (a.d < 1 || a.d > kBasketMax) return hipErrorInvalidValue;
    int vec = s.vec_hint >= 4 || s.vec_hint <= 0 ? 4 : s.vec_hint >= 2 ? 2 : 1;
    if (vec > basket_vec_cap(a.d)) vec = basket_vec_cap(a.d);
    // VEC-wide stores in both buffers (asset k's matrix starts k (N + 1) ld_assets floats in: aligned where its rows are)
    vec = store_vec_width(vec, P, s.S, s.ld);
    if (a.assets) vec = store_vec_width(vec, P, a.assets, a.ld_assets);
    if (a.assets && a.state) vec = store_vec_width(vec, P, a.state, a.ld_assets);
    BasketArgs g{};
    g.S = s.S; g.A = a.assets; g.C = a.assets ? a.state : nullptr; g.ld = s.ld; g.lda = a.ld_assets; g.P = P; g.n_steps = s.n_steps;
    g.k0 = (uint32_t)s.seed; g.k1 = (uint32_t)(s.seed >> 32); g.stream = s.stream; g.pair_offset = s.pair_offset;
    const bool keep = a.assets != nullptr;
    for_assets(a.d, [&](auto d) { launch_basket_d<d()>(st, g, a.law, keep, vec); });
    return hipGetLastError();
}

}  // namespace omc
