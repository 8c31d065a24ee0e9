// omc_jump.hip -- path generator with compound-Poisson lognormal jumps: Merton (GBM) and Bates (Heston), DESIGN.md
// section 15.
//
// jump_paths_kernel<MODEL, VEC> writes the full-storage path matrix the unchanged two-pass LSM sweeps then price.
// A lane owns VEC antithetic pairs.  The diffusion is that of gbm_paths_body / heston_pair_step<SCHEME>
// (omc_paths_dev.h): same Philox counters, same operations, at the compensated drift rate.  On top of it step t of a
// pair carries n jumps, n exact Poisson by inversion on integers: w = the top 24 bits of word (t-1) & 3 of the Philox
// block at counter (pair lo, pair hi, 0x40000000 | (t-1) >> 2, stream), n = #{k : w >= thr[k]} (include/omc.h).  Where
// n > 0 the log2 jump is
//     jl = fmaf(sqrtf(n) sj2, z_J, n mj2),   z_J = the first normal of the block at (pair lo, pair hi, 0xC0000000 | t, stream)
// and BOTH partners take it: GBM adds jl to the exponent of the step, Heston multiplies both spots by exp2(jl) after
// heston_pair_step (the variance is untouched).  A step with n = 0 executes the vanilla operations and nothing else.
//
// One count block serves four steps: GBM's own block cadence, two normal blocks of Heston.  The hot case is "no lane of
// this wave jumps on this step": one compare with thr[0] per pair, one ballot and a scalar branch.  The other 15
// compares, the size block and the extra exp2 sit behind that branch.  The thresholds and (mj2, sj2) come by value in
// the argument block: scalar registers, no table in memory.  No grid-stride loop, no LDS; every write is a VEC-wide
// vector store.
#include "omc_jump.h"
#include "omc_jump_dev.h"  // jump_log2
#include "omc_paths_dev.h"

namespace omc {

// MODEL 0 GBM, 1/2/3/4 Heston scheme 0/1/2/3.  VEC-wide stores: the launcher picks a VEC every row start is aligned to.
template <int MODEL, int VEC>
__global__ __launch_bounds__(kBlock) void jump_paths_kernel(PathArgs g, JumpLaw j)
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
    constexpr int NPC = 4 / SPB;             // blocks of normals per count block
    const int n_steps = g.n_steps;
    const int ncb = (n_steps + 3) >> 2;
    const uint32_t thr0 = j.thr[0];
    int t = 0;
    for (int cb = 0; cb < ncb; ++cb) {
        uint32_t w[VEC][4];  // the count words of steps 4 cb + 1 .. 4 cb + 4
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const uint64_t pair = g.pair_offset + (uint64_t)(p0 + v);
            const U4 o = philox4x32_10((uint32_t)pair, (uint32_t)(pair >> 32), 0x40000000u | (uint32_t)cb, g.stream, g.k0, g.k1);
            w[v][0] = o.x >> 8; w[v][1] = o.y >> 8; w[v][2] = o.z >> 8; w[v][3] = o.w >> 8;
        }
#pragma unroll
        for (int h = 0; h < NPC; ++h) {
            if (t >= n_steps) break;
            float z[VEC][4];
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                normals4(g.pair_offset + (uint64_t)(p0 + v), (uint32_t)(cb * NPC + h), g.stream, g.k0, g.k1, z[v]);
#pragma unroll
            for (int i = 0; i < SPB; ++i) {
                if (t >= n_steps) break;
                ++t;
                row += ld;
                const int ci = h * SPB + i;  // the step's word of the count block
                bool any = false;
#pragma unroll
                for (int v = 0; v < VEC; ++v) any |= w[v][ci] >= thr0;
                if (__builtin_amdgcn_ballot_w64(any) == 0) {  // no lane of the wave jumps: the vanilla step
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        if constexpr (MODEL == 0) {
                            s[v] = s[v] * fast_exp2(__builtin_fmaf(b, z[v][i], a));
                            sa[v] = sa[v] * fast_exp2(__builtin_fmaf(-b, z[v][i], a));
                        } else {
                            heston_pair_step<MODEL - 1>(g.hc, z[v][2 * i], z[v][2 * i + 1], s[v], va[v], sa[v], vb[v]);
                        }
                    }
                } else {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const bool jumps = w[v][ci] >= thr0;
                        float jl = 0.0f;
                        if (jumps) jl = jump_log2(j, w[v][ci], g.pair_offset + (uint64_t)(p0 + v), t, g.stream, g.k0, g.k1);
                        if constexpr (MODEL == 0) {
                            float e = __builtin_fmaf(b, z[v][i], a), ea = __builtin_fmaf(-b, z[v][i], a);
                            if (jumps) {
                                e += jl;
                                ea += jl;
                            }
                            s[v] = s[v] * fast_exp2(e);
                            sa[v] = sa[v] * fast_exp2(ea);
                        } else {
                            heston_pair_step<MODEL - 1>(g.hc, z[v][2 * i], z[v][2 * i + 1], s[v], va[v], sa[v], vb[v]);
                            if (jumps) {
                                const float f = fast_exp2(jl);
                                s[v] = s[v] * f;
                                sa[v] = sa[v] * f;
                            }
                        }
                    }
                }
                store_vec<VEC>(row, s);
                store_vec<VEC>(row + P, sa);
            }
        }
    }
}

hipError_t launch_jump_paths(hipStream_t st, const JumpGen& a)
{
    const PathSpec& s = a.paths;
    const int64_t P = s.n_paths / 2;
    if (P <= 0) return hipSuccess;
    const PathArgs g = make_path_args(s, P);
    const int width = store_vec_width(s.vec_hint, P, s.S, s.ld);  // (so P % VEC == 0 and every store is VEC wide)
    for_model(s.model, s.scheme, [&](auto model) {
        for_vec(width, [&](auto vec) {
            constexpr int MO = decltype(model)::value, V = decltype(vec)::value;
            hipLaunchKernelGGL((jump_paths_kernel<MO, V>), dim3((unsigned)((P / V + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                               g, a.law);
        });
    });
    return hipGetLastError();
}

}  // namespace omc
