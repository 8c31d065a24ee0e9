// omc_jump_bounds.hip -- Andersen-Broadie price bounds under jump-diffusion: Merton (GBM) and Bates (Heston), DESIGN.md
// section 28.
//
// The four sweeps that simulate fresh paths (bounds_lower_body, bounds_inner_body: omc_bounds_dev.h;
// bounds_sched_inner_body: omc_bounds_sched_dev.h; bounds_check_inner_body: omc_bounds_check_dev.h) with the jump law of
// omc_jump.hip as their Model, and the jump generator that keeps the variance state of the outer paths.
// Every spot is the jump generator's: the diffusion of gbm_paths_body / heston_pair_step<SCHEME> at the compensated drift
// rate from the pair's blocks of normals, and on top of it the step's n jumps -- n from word (t-1) & 3 of the pair's count
// block (t-1) >> 2, the size from the block at 0xC0000000 | t, both partners alike (include/omc.h, "jump-diffusion").
// The sweeps hand step() neither the pair nor the step number, so the law's Normals carry them: draw() knows the pair, the
// block of four steps and the stream, fetches the count block with the normals, and step u of the block is step
// 4 blk + u + 1 of the path.  A step keeps the generator's shape: one compare with thr[0] per lane, one ballot over the
// lanes that execute the step (inside the sweeps' divergent code the ballot covers exactly those), and a scalar branch:
// where no live lane jumps the vanilla step runs and nothing else.  The other 15 compares, the size block and the extra
// exp2 sit behind that branch.  The thresholds and (mj2, sj2) come by value in the argument block.
#include "omc_jump_bounds.h"

#include "omc_bounds_law_dev.h"
#include "omc_jump_dev.h"

namespace omc {

// what the jump-diffusion kernels take by value: the diffusion at the compensated drift rate and the jump law
struct JumpBoundsArgs {
    DiffusionArgs d;
    JumpLaw law;
};

// the jump path law (the Model of omc_bounds_dev.h) on the diffusion MODEL 0 GBM, 1 / 2 Heston scheme 0 / 1; the policy
// sees the spot
template <int MODEL>
struct JumpBoundsModel : DiffusionModel<MODEL> {
    using Base = DiffusionModel<MODEL>;
    using Args = JumpBoundsArgs;
    using Spots = typename Base::Spots;
    struct Normals {
        typename Base::Normals z;
        uint32_t w[4];  // the four steps' count words (top 24 bits)
        uint64_t pair;
        uint32_t blk, stream;
    };
    const Args& g;
    __device__ __forceinline__ JumpBoundsModel(const Args& g) : Base{g.d}, g(g) {}
    static __device__ __forceinline__ const BoundsArgs& common(const Args& g) { return g.d.v; }
    // four steps of generator pair `pair`: the diffusion's normals and count block blk
    __device__ __forceinline__ void draw(uint64_t pair, uint32_t blk, uint32_t stream, Normals& n) const
    {
        Base::draw(pair, blk, stream, n.z);
        const U4 o = philox4x32_10((uint32_t)pair, (uint32_t)(pair >> 32), 0x40000000u | blk, stream, g.d.v.k0, g.d.v.k1);
        n.w[0] = o.x >> 8; n.w[1] = o.y >> 8; n.w[2] = o.z >> 8; n.w[3] = o.w >> 8;
        n.pair = pair; n.blk = blk; n.stream = stream;
    }
    __device__ __forceinline__ void step(Spots& s, const Normals& n, int u) const
    {
        const bool jumps = n.w[u] >= g.law.thr[0];
        if (__builtin_amdgcn_ballot_w64(jumps) == 0) {  // no lane that takes this step jumps: the vanilla step
            Base::step(s, n.z, u);
        } else {
            float jl = 0.0f;
            if (jumps) jl = jump_log2(g.law, n.w[u], n.pair, (int)(4 * n.blk) + u + 1, n.stream, g.d.v.k0, g.d.v.k1);
            if constexpr (MODEL == 0) {  // the jump goes into the step's exponent
                const BoundsArgs& v = g.d.v;
                float e = __builtin_fmaf(v.b, n.z[u], v.a), eb = __builtin_fmaf(-v.b, n.z[u], v.a);
                if (jumps) {
                    e += jl;
                    eb += jl;
                }
                s.sa = s.sa * fast_exp2(e);
                s.sb = s.sb * fast_exp2(eb);
            } else {
                Base::step(s, n.z, u);
                if (jumps) {
                    const float f = fast_exp2(jl);
                    s.sa = s.sa * f;
                    s.sb = s.sb * f;
                }
            }
        }
    }
};

// ------------------------------------------------------------------ the generator that keeps the variance
// jump_paths_kernel<SCHEME + 1, 1> with V beside S: the same counters, the same steps, the same spots
template <int SCHEME>
__global__ __launch_bounds__(kBlock) void jump_paths_sv_kernel(PathArgs g, JumpLaw j, float* __restrict__ V)
{
    float* __restrict__ S = g.S;
    const int64_t ld = g.ld, P = g.P;
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= P) return;
    const uint64_t pair = g.pair_offset + (uint64_t)p;
    float s = g.s_init, sa = g.s_init, va = g.v_init, vb = g.v_init;
    int64_t at = p;
    S[at] = s;
    S[at + P] = sa;
    V[at] = va;
    V[at + P] = vb;
    const int n_steps = g.n_steps;
    const int ncb = (n_steps + 3) >> 2;
    const uint32_t thr0 = j.thr[0];
    int t = 0;
    for (int cb = 0; cb < ncb; ++cb) {
        const U4 o = philox4x32_10((uint32_t)pair, (uint32_t)(pair >> 32), 0x40000000u | (uint32_t)cb, g.stream, g.k0, g.k1);
        const uint32_t w[4] = {o.x >> 8, o.y >> 8, o.z >> 8, o.w >> 8};  // the count words of steps 4 cb + 1 .. 4 cb + 4
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (t >= n_steps) break;
            float z[4];
            normals4(pair, (uint32_t)(cb * 2 + h), g.stream, g.k0, g.k1, z);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (t >= n_steps) break;
                ++t;
                at += ld;
                const uint32_t wc = w[h * 2 + i];
                const bool jumps = wc >= thr0;
                heston_pair_step<SCHEME>(g.hc, z[2 * i], z[2 * i + 1], s, va, sa, vb);
                if (__builtin_amdgcn_ballot_w64(jumps) != 0) {  // (the vanilla step and nothing else where no lane jumps)
                    if (jumps) {
                        const float f = fast_exp2(jump_log2(j, wc, pair, t, g.stream, g.k0, g.k1));
                        s = s * f;
                        sa = sa * f;
                    }
                }
                S[at] = s;
                S[at + P] = sa;
                V[at] = va;
                V[at + P] = vb;
            }
        }
    }
}

// ------------------------------------------------------------------ launchers
hipError_t launch_jump_paths_sv(hipStream_t st, const JumpGen& a, float* V)
{
    return launch_paths_sv(a.paths, [&](auto sc, dim3 grid, dim3 block, const PathArgs& g) {
        hipLaunchKernelGGL((jump_paths_sv_kernel<decltype(sc)::value>), grid, block, 0, st, g, a.law, V);
    });
}

static JumpBoundsArgs jump_args(const BoundsArgs& a, const JumpBoundsLaw& l) { return {diffusion_args(a, l.d), l.law}; }

hipError_t bounds_lower(hipStream_t st, const BoundsArgs& a, const JumpBoundsLaw& l, double* result)
{
    return launch_bounds_lower<JumpBoundsModel, 0, 1, 2>(st, diffusion_model(l.d), a, jump_args(a, l), result);
}

hipError_t bounds_inner(hipStream_t st, const BoundsArgs& a, const JumpBoundsLaw& l, int64_t i0, int64_t ni)
{
    return launch_bounds_inner<JumpBoundsModel, 0, 1, 2>(st, diffusion_model(l.d), a, jump_args(a, l), i0, ni);
}

hipError_t bounds_sched_inner(hipStream_t st, const BoundsArgs& a, const JumpBoundsLaw& l, const BoundsSched& sc, int64_t i0,
                              int64_t ni)
{
    return launch_bounds_sched_inner<JumpBoundsModel, 0, 1, 2>(st, diffusion_model(l.d), a, jump_args(a, l), sc, i0, ni);
}

hipError_t bounds_check_inner(hipStream_t st, const BoundsArgs& a, const JumpBoundsLaw& l, const BoundsCheck& k, int64_t i0,
                              int64_t ni)
{
    return launch_bounds_check_inner<JumpBoundsModel, 0, 1, 2>(st, diffusion_model(l.d), a, jump_args(a, l), k, i0, ni);
}

}  // namespace omc
