// omc_heston_bounds.hip -- Andersen-Broadie price bounds under the Heston model.
//
// The two sweeps of omc_bounds.hip that simulate paths (bounds_lower_body, bounds_inner_body: omc_bounds_dev.h) with the
// Heston path law, and the generator that writes the outer paths WITH their variance state.
//   lower   one thread per antithetic pair of fresh paths, (s, v) of both partners in registers; each partner stops at
//           the first date the rule fires on its SPOT.
//   inner   the hot path: a wave per (outer path, date) item, a lane per antithetic inner pair.  The item's start state
//           (S_t[i], V_t[i]) is loaded once per item, wave-uniform.  A draw is two Philox blocks = four steps.
//   sv      heston_paths_body's spots (one pair per thread) with the variance of both partners stored after every step.
// Every spot is the Heston generator's (omc_paths_dev.h): heston_pair_step<SCHEME> on the normals of normals4(pair, block
// k of two steps), the partner with (-z1, -z2).  The policy sees the spot alone; the outer walk, the exercise tables and
// the finalize are omc_bounds.hip's / omc_lsm.hip's.
#include "omc_heston_bounds.h"

#include "omc_bounds_check_dev.h"
#include "omc_bounds_dev.h"
#include "omc_bounds_sched_dev.h"
#include "omc_paths_dev.h"

namespace omc {

// what the Heston kernels take by value: the common arguments and the law's float32 constants
struct HestonBoundsArgs {
    BoundsArgs v;
    HestonC hc;
    float v0;         // (float)v0: the variance every lower pair starts at
    const float* Vo;  // [N+1][n_outer] variance state of the outer paths
};

// the Heston path law (the Model of omc_bounds_dev.h); the policy sees the spot
template <int SCHEME>
struct HestonBoundsModel {
    struct Start { float s, v; };
    struct Spots { float sa, sb, va, vb; };
    using Normals = float[8];
    const HestonBoundsArgs& g;
    __device__ __forceinline__ Start lower_start() const { return Start{g.v.s0, g.v0}; }
    // the outer state (S_t[i], V_t[i]): one address per wave, held as scalars
    __device__ __forceinline__ Start inner_start(int t, int64_t i) const
    {
        const size_t at = (size_t)t * g.v.n_outer + i;
        Start s0;
        s0.s = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(g.v.So[at])));
        s0.v = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(g.Vo[at])));
        return s0;
    }
    __device__ __forceinline__ void reset(Spots& s, const Start& s0) const
    {
        s.sa = s.sb = s0.s;
        s.va = s.vb = s0.v;
    }
    // four steps: the generator's blocks 2 blk and 2 blk + 1 (one Philox block per two steps)
    __device__ __forceinline__ void draw(uint64_t pair, uint32_t blk, uint32_t stream, Normals& z) const
    {
        normals4(pair, 2 * blk, stream, g.v.k0, g.v.k1, reinterpret_cast<float(&)[4]>(z[0]));
        normals4(pair, 2 * blk + 1, stream, g.v.k0, g.v.k1, reinterpret_cast<float(&)[4]>(z[4]));
    }
    __device__ __forceinline__ void step(Spots& s, const Normals& z, int u) const
    {
        heston_pair_step<SCHEME>(g.hc, z[2 * u], z[2 * u + 1], s.sa, s.va, s.sb, s.vb);
    }
    __device__ __forceinline__ float index_a(const Spots& s) const { return s.sa; }
    __device__ __forceinline__ float index_b(const Spots& s) const { return s.sb; }
};

template <int SCHEME>
__global__ __launch_bounds__(kBlock) void heston_bounds_lower_kernel(HestonBoundsArgs g, int nblk)
{
    extern __shared__ uint4 sh_bt[];
    __shared__ double red[kNQ * kRedStride];
    bounds_lower_body(g.v, HestonBoundsModel<SCHEME>{g}, nblk, sh_bt, red);
}

template <int SCHEME>
__global__ __launch_bounds__(kBlock) void heston_bounds_inner_kernel(HestonBoundsArgs g, int64_t i0, int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bounds_inner_body(g.v, HestonBoundsModel<SCHEME>{g}, i0, ni, sh_bt);
}

// the inner sweep of an exercise schedule (omc_bounds_sched_dev.h) under the Heston law
template <int SCHEME>
__global__ __launch_bounds__(kBlock) void heston_bounds_sched_inner_kernel(HestonBoundsArgs g, BoundsSched sc, int64_t i0,
                                                                           int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bounds_sched_inner_body(g.v, sc, HestonBoundsModel<SCHEME>{g}, i0, ni, sh_bt);
}

// the list-driven inner sweep of sub-optimality checking (omc_bounds_check_dev.h) under the Heston law
template <int SCHEME>
__global__ __launch_bounds__(kBlock) void heston_bounds_check_inner_kernel(HestonBoundsArgs g, BoundsCheck k, int64_t i0,
                                                                           int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bounds_check_inner_body(g.v, k, HestonBoundsModel<SCHEME>{g}, i0, ni, sh_bt);
}

// ------------------------------------------------------------------ the generator that keeps the variance
// heston_paths_body<1, SCHEME> with V beside S: the same counters, the same steps, the same spots
template <int SCHEME>
__global__ __launch_bounds__(kBlock) void heston_paths_sv_kernel(PathArgs g, float* __restrict__ V)
{
    float* __restrict__ S = g.S;
    const int64_t ld = g.ld, P = g.P;
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= P) return;
    float s = g.s_init, sa = g.s_init, va = g.v_init, vb = g.v_init;
    int64_t at = p;
    S[at] = s;
    S[at + P] = sa;
    V[at] = va;
    V[at + P] = vb;
    const int nblk = (g.n_steps + 1) >> 1;
    int t = 0;
    for (int blk = 0; blk < nblk; ++blk) {
        float z[4];
        normals4(g.pair_offset + (uint64_t)p, (uint32_t)blk, g.stream, g.k0, g.k1, z);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (++t > g.n_steps) break;
            at += ld;
            heston_pair_step<SCHEME>(g.hc, z[2 * i], z[2 * i + 1], s, va, sa, vb);
            S[at] = s;
            S[at + P] = sa;
            V[at] = va;
            V[at + P] = vb;
        }
    }
}

// ------------------------------------------------------------------ launchers
hipError_t launch_heston_paths_sv(hipStream_t st, float* S, float* V, int64_t ld, int64_t n_paths, int n_steps, double S0,
                                  double r, double T, double v0, double kappa, double theta, double xi, double rho,
                                  uint64_t seed, uint32_t stream, uint64_t pair_offset, int scheme)
{
    PathSpec s{};
    s.model = 1; s.scheme = scheme; s.n_paths = n_paths; s.n_steps = n_steps; s.S0 = S0; s.r = r; s.T = T;
    s.v0 = v0; s.kappa = kappa; s.theta = theta; s.xi = xi; s.rho = rho;
    s.seed = seed; s.pair_offset = pair_offset; s.stream = stream; s.S = S; s.ld = ld;
    const int64_t P = n_paths / 2;
    if (P <= 0) return hipSuccess;
    const PathArgs g = make_path_args(s, P);
    const dim3 grid((unsigned)((P + kBlock - 1) / kBlock)), block(kBlock);
    if (scheme < 0 || scheme > 3) return hipErrorInvalidValue;
    for_scheme(scheme, [&](auto sc) {
        hipLaunchKernelGGL((heston_paths_sv_kernel<decltype(sc)::value>), grid, block, 0, st, g, V);
    });
    return hipGetLastError();
}

static HestonBoundsArgs heston_bounds_args(const BoundsArgs& a, const HestonBoundsLaw& h)
{
    HestonBoundsArgs g{};
    g.v = a;
    g.hc = make_heston(h.r, h.T, a.N, h.kappa, h.theta, h.xi, h.rho);
    g.v0 = (float)h.v0;
    g.Vo = h.Vo;
    return g;
}

hipError_t heston_bounds_lower(hipStream_t st, const BoundsArgs& a, const HestonBoundsLaw& h, double* result)
{
    if (h.scheme != 0 && h.scheme != 1) return hipErrorInvalidValue;
    const HestonBoundsArgs g = heston_bounds_args(a, h);
    const int nblk = (int)bounds_lower_blocks(a);  // the vanilla sweep's grid
    const size_t lds = sizeof(uint4) * (size_t)(a.N + 1);
    if (h.scheme == 0) hipLaunchKernelGGL((heston_bounds_lower_kernel<0>), dim3(nblk), dim3(kBlock), lds, st, g, nblk);
    else hipLaunchKernelGGL((heston_bounds_lower_kernel<1>), dim3(nblk), dim3(kBlock), lds, st, g, nblk);
    return lsm_finalize(st, a.part, nullptr, result, nblk, 0);
}

hipError_t heston_bounds_inner(hipStream_t st, const BoundsArgs& a, const HestonBoundsLaw& h, int64_t i0, int64_t ni)
{
    if (h.scheme != 0 && h.scheme != 1) return hipErrorInvalidValue;
    const HestonBoundsArgs g = heston_bounds_args(a, h);
    const int64_t items = ni * a.N;
    int64_t nb = (items + 3) / 4;
    if (nb > 2048) nb = 2048;
    const size_t lds = sizeof(uint4) * (size_t)(a.N + 1);
    if (h.scheme == 0)
        hipLaunchKernelGGL((heston_bounds_inner_kernel<0>), dim3((unsigned)nb), dim3(kBlock), lds, st, g, i0, ni);
    else
        hipLaunchKernelGGL((heston_bounds_inner_kernel<1>), dim3((unsigned)nb), dim3(kBlock), lds, st, g, i0, ni);
    return hipGetLastError();
}

hipError_t heston_bounds_sched_inner(hipStream_t st, const BoundsArgs& a, const HestonBoundsLaw& h, const BoundsSched& sc,
                                     int64_t i0, int64_t ni)
{
    if ((h.scheme != 0 && h.scheme != 1) || !bounds_schedule_ok(sc, a.N)) return hipErrorInvalidValue;
    const HestonBoundsArgs g = heston_bounds_args(a, h);
    const int64_t items = ni * sc.J;
    int64_t nb = (items + 3) / 4;
    if (nb > 2048) nb = 2048;
    const size_t lds = sizeof(uint4) * (size_t)(a.N + 1);
    if (h.scheme == 0)
        hipLaunchKernelGGL((heston_bounds_sched_inner_kernel<0>), dim3((unsigned)nb), dim3(kBlock), lds, st, g, sc, i0, ni);
    else
        hipLaunchKernelGGL((heston_bounds_sched_inner_kernel<1>), dim3((unsigned)nb), dim3(kBlock), lds, st, g, sc, i0, ni);
    return hipGetLastError();
}

hipError_t heston_bounds_check_inner(hipStream_t st, const BoundsArgs& a, const HestonBoundsLaw& h, const BoundsCheck& k,
                                     int64_t i0, int64_t ni)
{
    if (h.scheme != 0 && h.scheme != 1) return hipErrorInvalidValue;
    const HestonBoundsArgs g = heston_bounds_args(a, h);
    const int64_t items = ni * a.N;  // the dense sweep's grid: the kept items are a subset
    int64_t nb = (items + 3) / 4;
    if (nb > 2048) nb = 2048;
    const size_t lds = sizeof(uint4) * (size_t)(a.N + 1);
    if (h.scheme == 0)
        hipLaunchKernelGGL((heston_bounds_check_inner_kernel<0>), dim3((unsigned)nb), dim3(kBlock), lds, st, g, k, i0, ni);
    else
        hipLaunchKernelGGL((heston_bounds_check_inner_kernel<1>), dim3((unsigned)nb), dim3(kBlock), lds, st, g, k, i0, ni);
    return hipGetLastError();
}

}  // namespace omc
