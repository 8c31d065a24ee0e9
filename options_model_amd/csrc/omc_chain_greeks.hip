// omc_chain_greeks.hip -- the Greeks of an option chain's entries: the sweep of omc_greeks.hip for
// up to 16 entries of one side in ONE launch, and the two small launches around it with the entry on grid.y.
//
//   lsm_greeks_chain_kernel         a workgroup is one (column block, entry) pair and runs greeks_body (omc_greeks_dev.h) on
//                                   the entry's view with the view's step map; its partials land at [entry][q][column block],
//                                   so an entry's sums are the single kernel's, added in the single kernel's order
//   lsm_solve_betas_group_kernel    lsm_solve_betas_kernel's body per member
//   lsm_greeks_finalize_group_kernel  lsm_greeks_finalize_kernel's body per member
// The per-entry data is read from a slot array in device memory (ChainGreeksSlot): uniform per workgroup, so scalar loads.
#include "omc_chain_greeks.h"
#include "omc_greeks_dev.h"

namespace omc {

// the (column block, entry) pair of linear workgroup index L of an nblk x E grid (omc_chain_greeks.h: both orders are
// bijections onto [0, nblk) x [0, E))
__device__ __forceinline__ void chain_greeks_block(int64_t L, int64_t nblk, int E, int order, int64_t* blk, int* e)
{
    if (order == kChainGreeksPlain) {
        *e = (int)(L / nblk);
        *blk = L - (int64_t)*e * nblk;
        return;
    }
    // bands of 8 column blocks; every band before the last is full, the last holds nblk - 8 b of them
    const int64_t b = L / (8 * (int64_t)E);
    const int64_t rest = nblk - 8 * b;
    const int w = (int)(rest < 8 ? rest : 8);
    const int r = (int)(L - 8 * (int64_t)E * b);  // < w E
    *e = r / w;
    *blk = 8 * b + (r - *e * w);
}

template <int VEC, bool FOLD, int PUT>
__global__ __launch_bounds__(kBlock) void lsm_greeks_chain_kernel(ChainGreeksArgs c, int first, int E)
{
    int64_t blk;
    int e;
    chain_greeks_block(blockIdx.x, c.nblk, E, c.order, &blk, &e);
    const ChainGreeksSlot& s = c.slots[first + e];
    GreeksArgs a;
    a.S = s.S; a.ld = s.ld; a.cols = c.cols;
    a.N = s.N; a.is_put = PUT; a.gbm = c.gbm;
    a.K = s.K; a.S0 = c.S0; a.r = c.r; a.sigma = c.sigma; a.T = c.T; a.h = c.h;
    a.D = s.D; a.betas = s.betas; a.cK = s.cK; a.gmom = nullptr;
    a.part = s.part; a.result = nullptr;
    greeks_body<VEC, FOLD, PUT>(a, GreeksViewGrid{blk, (size_t)c.nblk, s.every, c.Nf});
}

__global__ void lsm_solve_betas_group_kernel(ChainGreeksArgs c)
{
    const ChainGreeksSlot& s = c.slots[blockIdx.y];
    if (s.gmom) lsm_solve_all_body(s.gmom, s.betas, s.N);  // (steps past the member's own return at once)
}

__global__ __launch_bounds__(kBlock) void lsm_greeks_finalize_group_kernel(ChainGreeksArgs c)
{
    const ChainGreeksSlot& s = c.slots[blockIdx.y];
    greeks_finalize_body(s.part, c.nblk, s.gmom, s.N, s.result, blockIdx.x);
}

hipError_t chain_greeks_sweep(hipStream_t st, const ChainGreeksArgs& a, int first, int E, int is_put, bool folded, int n_max)
{
    if (E < 1 || E > kChainGreeksMax || a.nblk < 1 || a.nblk * E > 0x7fffffffLL) return hipErrorInvalidValue;
    const size_t dyn = sizeof(double) * 4 * (size_t)(n_max + 1);
    for_int<2, 1>(a.vec, [&](auto vec) {
        for_flag(folded, [&](auto fold) {
            for_put(is_put, [&](auto put) {
                constexpr int VEC = decltype(vec)::value, PUT = decltype(put)::value;
                hipLaunchKernelGGL((lsm_greeks_chain_kernel<VEC, decltype(fold)::value, PUT>), dim3((unsigned)(a.nblk * E)),
                                   dim3(kBlock), dyn, st, a, first, E);
            });
        });
    });
    return hipGetLastError();
}

hipError_t chain_greeks_solve(hipStream_t st, const ChainGreeksArgs& a, int E, int n_max)
{
    if (n_max < 2) return hipSuccess;
    hipLaunchKernelGGL(lsm_solve_betas_group_kernel, dim3((n_max + kBlock - 1) / kBlock, E), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t chain_greeks_finalize(hipStream_t st, const ChainGreeksArgs& a, int E)
{
    hipLaunchKernelGGL(lsm_greeks_finalize_group_kernel, dim3(3, E), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace omc
