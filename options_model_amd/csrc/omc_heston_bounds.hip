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
// the finalize are omc_bounds.hip's / omc_lsm.hip's.  The law adds nothing to the shared diffusion: its Model is
// DiffusionModel<1> / <2> (omc_bounds_law_dev.h), its argument block DiffusionArgs, its kernels that file's wrappers.
#include "omc_heston_bounds.h"

#include "omc_bounds_law_dev.h"

namespace omc {

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
hipError_t launch_heston_paths_sv(hipStream_t st, const PathSpec& s, float* V)
{
    return launch_paths_sv(s, [&](auto sc, dim3 grid, dim3 block, const PathArgs& g) {
        hipLaunchKernelGGL((heston_paths_sv_kernel<decltype(sc)::value>), grid, block, 0, st, g, V);
    });
}

// (a GBM law has no kernels here: model number 0 is not listed)
hipError_t bounds_lower(hipStream_t st, const BoundsArgs& a, const DiffusionLaw& h, double* result)
{
    return launch_bounds_lower<DiffusionModel, 1, 2>(st, diffusion_model(h), a, diffusion_args(a, h), result);
}

hipError_t bounds_inner(hipStream_t st, const BoundsArgs& a, const DiffusionLaw& h, int64_t i0, int64_t ni)
{
    return launch_bounds_inner<DiffusionModel, 1, 2>(st, diffusion_model(h), a, diffusion_args(a, h), i0, ni);
}

hipError_t bounds_sched_inner(hipStream_t st, const BoundsArgs& a, const DiffusionLaw& h, const BoundsSched& sc, int64_t i0,
                              int64_t ni)
{
    return launch_bounds_sched_inner<DiffusionModel, 1, 2>(st, diffusion_model(h), a, diffusion_args(a, h), sc, i0, ni);
}

hipError_t bounds_check_inner(hipStream_t st, const BoundsArgs& a, const DiffusionLaw& h, const BoundsCheck& k, int64_t i0,
                              int64_t ni)
{
    return launch_bounds_check_inner<DiffusionModel, 1, 2>(st, diffusion_model(h), a, diffusion_args(a, h), k, i0, ni);
}

}  // namespace omc
