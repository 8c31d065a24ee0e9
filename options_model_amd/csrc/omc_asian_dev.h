// omc_asian_dev.h -- the path law of the running-average (Asian) index kinds for the bound kernels (DESIGN.md section 23;
// the definitions are include/omc.h's): D correlated GBM assets as omc_basket_dev.h steps them, and beside either partner's
// spots the running state of the generator (omc_basket.hip) -- c_t, the float32 sum of the basket values B_1 .. B_t
// (OMC_BASKET_ASIAN_ARITHMETIC), or l_t, the sum of their hardware log2 (OMC_BASKET_ASIAN_GEOMETRIC).
//
// It is a Model of omc_bounds_dev.h (index_a / index_b: the average) and of omc_bounds2_dev.h (xy_a / xy_b / xy_outer: the
// average and the current basket value B_t).  Neither body passes a date to `step`, and the rule of step n divides by n,
// so Spots carries its own step counter: `reset` sets it from Start, which an inner item fills with its date t and the
// outer path's stored state -- the state the generator wrote, never X_t * t.  Every operation is the generator's, in its
// order: the same bits for the arithmetic kind, the same instructions for the geometric one.
#pragma once
#include "omc_basket_bounds.h"
#include "omc_basket_dev.h"
#include "omc_bounds2_dev.h"

namespace omc {

template <int D>
struct AsianModel {
    struct Start {
        float v[D];  // asset spots
        float c;     // running state at the start
        int t;       // dates already in the state
    };
    struct Spots {
        float a[D], b[D];  // both partners' asset spots
        float ca, cb;      // ... running states
        float Ba, Bb;      // ... basket values of the last step
        float inv;         // 1.0f / n, correctly rounded
        int n;             // dates in the state
    };
    using Normals = float[D][4];
    const BasketBoundsArgs& g;

    __device__ __forceinline__ Start lower_start() const
    {
        Start s0;
#pragma unroll
        for (int k = 0; k < D; ++k) s0.v[k] = g.law.s0[k];
        s0.c = 0.0f;
        s0.t = 0;
        return s0;
    }
    // the outer asset spots A_k[t][i] and the outer running state C[t][i]: one address per wave, held as scalars
    __device__ __forceinline__ Start inner_start(int t, int64_t i) const
    {
        const size_t astride = (size_t)(g.v.N + 1) * (size_t)g.v.n_outer;  // one asset's outer matrix
        const size_t at = (size_t)t * g.v.n_outer + i;
        Start s0;
#pragma unroll
        for (int k = 0; k < D; ++k)
            s0.v[k] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(g.Ao[(size_t)k * astride + at])));
        s0.c = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(g.Co[at])));
        s0.t = t;
        return s0;
    }
    __device__ __forceinline__ void reset(Spots& s, const Start& s0) const
    {
#pragma unroll
        for (int k = 0; k < D; ++k) s.a[k] = s.b[k] = s0.v[k];
        s.ca = s.cb = s0.c;
        s.Ba = s.Bb = 0.0f;
        s.inv = 1.0f;
        s.n = s0.t;
    }
    __device__ __forceinline__ void draw(uint64_t pair, uint32_t blk, uint32_t stream, Normals& y) const
    {
        basket_normals<D>(g.law, pair, blk, stream, g.v.k0, g.v.k1, y);
    }
    __device__ __forceinline__ void step(Spots& s, const Normals& y, int u) const
    {
        basket_step<D>(g.law, s.a, s.b, y, u);
        s.n += 1;
        s.inv = __fdiv_rn(1.0f, (float)s.n);
        s.Ba = basket_index<OMC_BASKET_ARITHMETIC, D>(g.law, s.a);
        s.Bb = basket_index<OMC_BASKET_ARITHMETIC, D>(g.law, s.b);
        if (g.law.kind == OMC_BASKET_ASIAN_ARITHMETIC) {  // (wave-uniform: a scalar branch)
            s.ca = asian_add(s.ca, s.Ba);
            s.cb = asian_add(s.cb, s.Bb);
        } else {
            s.ca = s.ca + __builtin_amdgcn_logf(s.Ba);
            s.cb = s.cb + __builtin_amdgcn_logf(s.Bb);
        }
    }
    __device__ __forceinline__ float average(float c, float inv) const
    {
        return g.law.kind == OMC_BASKET_ASIAN_ARITHMETIC ? c * inv : fast_exp2(c * inv);
    }
    __device__ __forceinline__ float index_a(const Spots& s) const { return average(s.ca, s.inv); }
    __device__ __forceinline__ float index_b(const Spots& s) const { return average(s.cb, s.inv); }
    // the two regressors: the average and the basket value of the date
    __device__ __forceinline__ Pair2 xy_a(const Spots& s) const { return {average(s.ca, s.inv), s.Ba}; }
    __device__ __forceinline__ Pair2 xy_b(const Spots& s) const { return {average(s.cb, s.inv), s.Bb}; }
    // ... of outer path i at date t: the stored average and B_t from the stored asset spots (the generator's fmaf chain)
    __device__ __forceinline__ Pair2 xy_outer(int t, int64_t i) const
    {
        const size_t astride = (size_t)(g.v.N + 1) * (size_t)g.v.n_outer;
        const size_t at = (size_t)t * g.v.n_outer + i;
        float s[D];
#pragma unroll
        for (int k = 0; k < D; ++k) s[k] = g.Ao[(size_t)k * astride + at];
        return {g.v.So[at], basket_index<OMC_BASKET_ARITHMETIC, D>(g.law, s)};
    }
};

}  // namespace omc
