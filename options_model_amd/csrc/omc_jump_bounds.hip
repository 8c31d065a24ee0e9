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

#include "omc_bounds_check_dev.h"
#include "omc_bounds_dev.h"
#include "omc_bounds_sched_dev.h"
#include "omc_jump_dev.h"
#include "omc_paths_dev.h"

namespace omc {

// what the jump-diffusion kernels take by value: the common arguments (v.a, v.b: the GBM step constants at the drift
// rate), the Heston law's float32 constants at the drift rate, and the jump law
struct JumpBoundsArgs {
    BoundsArgs v;
    HestonC hc;
    float v0;         // (float)v0: the variance every lower pair starts at
    const float* Vo;  // [N+1][n_outer] variance state of the outer paths (Heston)
    JumpLaw law;
};

// the jump path law (the Model of omc_bounds_dev.h); MODEL 0 GBM, 1 / 2 Heston scheme 0 / 1; the policy sees the spot
template <int MODEL>
struct JumpBoundsModel {
    struct Start { float s, v; };
    struct Spots { float sa, sb, va, vb; };  // (GBM: va, vb are never read)
    struct Normals {
        float z[MODEL == 0 ? 4 : 8];  // four steps: one block of GBM, two of Heston
        uint32_t w[4];                // their count words (top 24 bits)
        uint64_t pair;
        uint32_t blk, stream;
    };
    const JumpBoundsArgs& g;
    __device__ __forceinline__ Start lower_start() const { return Start{g.v.s0, g.v0}; }
    // the outer state (S_t[i], V_t[i]): one address per wave, held as scalars
    __device__ __forceinline__ Start inner_start(int t, int64_t i) const
    {
        const size_t at = (size_t)t * g.v.n_outer + i;
        Start s0;
        s0.s = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(g.v.So[at])));
        if constexpr (MODEL == 0) s0.v = 0.0f;
        else s0.v = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(g.Vo[at])));
        return s0;
    }
    __device__ __forceinline__ void reset(Spots& s, const Start& s0) const
    {
        s.sa = s.sb = s0.s;
        s.va = s.vb = s0.v;
    }
    // four steps of generator pair `pair`: its normals (GBM block blk; Heston blocks 2 blk and 2 blk + 1) and count block blk
    __device__ __forceinline__ void draw(uint64_t pair, uint32_t blk, uint32_t stream, Normals& n) const
    {
        if constexpr (MODEL == 0) {
            normals4(pair, blk, stream, g.v.k0, g.v.k1, n.z);
        } else {
            normals4(pair, 2 * blk, stream, g.v.k0, g.v.k1, reinterpret_cast<float(&)[4]>(n.z[0]));
            normals4(pair, 2 * blk + 1, stream, g.v.k0, g.v.k1, reinterpret_cast<float(&)[4]>(n.z[4]));
        }
        const U4 o = philox4x32_10((uint32_t)pair, (uint32_t)(pair >> 32), 0x40000000u | blk, stream, g.v.k0, g.v.k1);
        n.w[0] = o.x >> 8; n.w[1] = o.y >> 8; n.w[2] = o.z >> 8; n.w[3] = o.w >> 8;
        n.pair = pair; n.blk = blk; n.stream = stream;
    }
    __device__ __forceinline__ void step(Spots& s, const Normals& n, int u) const
    {
        const bool jumps = n.w[u] >= g.law.thr[0];
        if (__builtin_amdgcn_ballot_w64(jumps) == 0) {  // no lane that takes this step jumps: the vanilla step
            if constexpr (MODEL == 0) {
                s.sa = s.sa * fast_exp2(__builtin_fmaf(g.v.b, n.z[u], g.v.a));
                s.sb = s.sb * fast_exp2(__builtin_fmaf(-g.v.b, n.z[u], g.v.a));
            } else {
                heston_pair_step<MODEL - 1>(g.hc, n.z[2 * u], n.z[2 * u + 1], s.sa, s.va, s.sb, s.vb);
            }
        } else {
            float jl = 0.0f;
            if (jumps) jl = jump_log2(g.law, n.w[u], n.pair, (int)(4 * n.blk) + u + 1, n.stream, g.v.k0, g.v.k1);
            if constexpr (MODEL == 0) {
                float e = __builtin_fmaf(g.v.b, n.z[u], g.v.a), eb = __builtin_fmaf(-g.v.b, n.z[u], g.v.a);
                if (jumps) {
                    e += jl;
                    eb += jl;
                }
                s.sa = s.sa * fast_exp2(e);
                s.sb = s.sb * fast_exp2(eb);
            } else {
                heston_pair_step<MODEL - 1>(g.hc, n.z[2 * u], n.z[2 * u + 1], s.sa, s.va, s.sb, s.vb);
                if (jumps) {
                    const float f = fast_exp2(jl);
                    s.sa = s.sa * f;
                    s.sb = s.sb * f;
                }
            }
        }
    }
    __device__ __forceinline__ float index_a(const Spots& s) const { return s.sa; }
    __device__ __forceinline__ float index_b(const Spots& s) const { return s.sb; }
};

template <int MODEL>
__global__ __launch_bounds__(kBlock) void jump_bounds_lower_kernel(JumpBoundsArgs g, int nblk)
{
    extern __shared__ uint4 sh_bt[];
    __shared__ double red[kNQ * kRedStride];
    bounds_lower_body(g.v, JumpBoundsModel<MODEL>{g}, nblk, sh_bt, red);
}

template <int MODEL>
__global__ __launch_bounds__(kBlock) void jump_bounds_inner_kernel(JumpBoundsArgs g, int64_t i0, int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bounds_inner_body(g.v, JumpBoundsModel<MODEL>{g}, i0, ni, sh_bt);
}

// the inner sweep of an exercise schedule (omc_bounds_sched_dev.h) under the jump law
template <int MODEL>
__global__ __launch_bounds__(kBlock) void jump_bounds_sched_inner_kernel(JumpBoundsArgs g, BoundsSched sc, int64_t i0,
                                                                         int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bounds_sched_inner_body(g.v, sc, JumpBoundsModel<MODEL>{g}, i0, ni, sh_bt);
}

// the list-driven inner sweep of sub-optimality checking (omc_bounds_check_dev.h) under the jump law
template <int MODEL>
__global__ __launch_bounds__(kBlock) void jump_bounds_check_inner_kernel(JumpBoundsArgs g, BoundsCheck k, int64_t i0,
                                                                         int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bounds_check_inner_body(g.v, k, JumpBoundsModel<MODEL>{g}, i0, ni, sh_bt);
}

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
    const PathSpec& s = a.paths;
    const int64_t P = s.n_paths / 2;
    if (P <= 0) return hipSuccess;
    if (s.model != 1 || s.scheme < 0 || s.scheme > 3) return hipErrorInvalidValue;
    const PathArgs g = make_path_args(s, P);
    const dim3 grid((unsigned)((P + kBlock - 1) / kBlock)), block(kBlock);
    for_scheme(s.scheme, [&](auto sc) {
        hipLaunchKernelGGL((jump_paths_sv_kernel<decltype(sc)::value>), grid, block, 0, st, g, a.law, V);
    });
    return hipGetLastError();
}

// the kernels' model number, or -1 for a law that has none
static int jump_bounds_model(const JumpBoundsLaw& l)
{
    if (l.model == 0) return 0;
    return l.model == 1 && (l.scheme == 0 || l.scheme == 1) ? l.scheme + 1 : -1;
}

static JumpBoundsArgs jump_bounds_args(const BoundsArgs& a, const JumpBoundsLaw& l)
{
    JumpBoundsArgs g{};
    g.v = a;
    if (l.model == 0) gbm_step_constants(l.drift_rate, l.sigma, l.T, a.N, &g.v.a, &g.v.b);
    else g.hc = make_heston(l.drift_rate, l.T, a.N, l.kappa, l.theta, l.xi, l.rho);
    g.v0 = (float)l.v0;
    g.Vo = l.Vo;
    g.law = l.law;
    return g;
}

// the inner sweeps' grid: four item waves per workgroup, at most 2048 workgroups (bounds_inner's)
static unsigned inner_grid(int64_t items)
{
    const int64_t nb = (items + 3) / 4;
    return (unsigned)(nb > 2048 ? 2048 : nb);
}

hipError_t jump_bounds_lower(hipStream_t st, const BoundsArgs& a, const JumpBoundsLaw& l, double* result)
{
    const int mo = jump_bounds_model(l);
    if (mo < 0) return hipErrorInvalidValue;
    const JumpBoundsArgs g = jump_bounds_args(a, l);
    const int nblk = (int)bounds_lower_blocks(a);  // the vanilla sweep's grid
    const size_t lds = sizeof(uint4) * (size_t)(a.N + 1);
    for_int<0, 1, 2>(mo, [&](auto model) {
        hipLaunchKernelGGL((jump_bounds_lower_kernel<decltype(model)::value>), dim3(nblk), dim3(kBlock), lds, st, g, nblk);
    });
    return lsm_finalize(st, a.part, nullptr, result, nblk, 0);
}

hipError_t jump_bounds_inner(hipStream_t st, const BoundsArgs& a, const JumpBoundsLaw& l, int64_t i0, int64_t ni)
{
    const int mo = jump_bounds_model(l);
    if (mo < 0) return hipErrorInvalidValue;
    const JumpBoundsArgs g = jump_bounds_args(a, l);
    const size_t lds = sizeof(uint4) * (size_t)(a.N + 1);
    for_int<0, 1, 2>(mo, [&](auto model) {
        hipLaunchKernelGGL((jump_bounds_inner_kernel<decltype(model)::value>), dim3(inner_grid(ni * a.N)), dim3(kBlock), lds,
                           st, g, i0, ni);
    });
    return hipGetLastError();
}

hipError_t jump_bounds_sched_inner(hipStream_t st, const BoundsArgs& a, const JumpBoundsLaw& l, const BoundsSched& sc,
                                   int64_t i0, int64_t ni)
{
    const int mo = jump_bounds_model(l);
    if (mo < 0 || !bounds_schedule_ok(sc, a.N)) return hipErrorInvalidValue;
    const JumpBoundsArgs g = jump_bounds_args(a, l);
    const size_t lds = sizeof(uint4) * (size_t)(a.N + 1);
    for_int<0, 1, 2>(mo, [&](auto model) {
        hipLaunchKernelGGL((jump_bounds_sched_inner_kernel<decltype(model)::value>), dim3(inner_grid(ni * sc.J)),
                           dim3(kBlock), lds, st, g, sc, i0, ni);
    });
    return hipGetLastError();
}

hipError_t jump_bounds_check_inner(hipStream_t st, const BoundsArgs& a, const JumpBoundsLaw& l, const BoundsCheck& k,
                                   int64_t i0, int64_t ni)
{
    const int mo = jump_bounds_model(l);
    if (mo < 0) return hipErrorInvalidValue;
    const JumpBoundsArgs g = jump_bounds_args(a, l);
    const size_t lds = sizeof(uint4) * (size_t)(a.N + 1);
    // the dense sweep's grid: the kept items are a subset
    for_int<0, 1, 2>(mo, [&](auto model) {
        hipLaunchKernelGGL((jump_bounds_check_inner_kernel<decltype(model)::value>), dim3(inner_grid(ni * a.N)), dim3(kBlock),
                           lds, st, g, k, i0, ni);
    });
    return hipGetLastError();
}

}  // namespace omc
