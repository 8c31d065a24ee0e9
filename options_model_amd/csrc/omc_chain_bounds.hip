// omc_chain_bounds.hip -- Andersen-Broadie price bounds of a whole option chain from one set of fresh paths (DESIGN.md
// section 33).
//
// The lower sweep and the inner simulations of omc_bounds.hip / omc_heston_bounds.hip, each with up to kChainBoundsMax frozen
// policies evaluated on ONE simulation of every path (chain_bounds_lower_body, chain_bounds_inner_body:
// omc_chain_bounds_dev.h).  The path law is the shared diffusion's Model (DiffusionModel<0> GBM, <1> / <2> Heston scheme
// 0 / 1: omc_bounds_law_dev.h) with its own start, reset, draw, step and index, so every spot is the generator's and every
// entry's stops are those of its single call.  The kernels are templates on the Model and on the number of entries E, whose
// per-entry state -- stop indices, stop dates, sums -- then lives in registers; a group shorter than the cap runs the kernel
// of its own length.  The outer paths, the exercise tables, the walk and the finalize are the single call's.
#include "omc_chain_bounds_dev.h"

#include "omc_bounds_law_dev.h"

namespace omc {

// what the chain kernels take by value: the diffusion's block first (the Models read it), then the group
struct ChainBoundsArgs {
    DiffusionArgs d;
    ChainBoundsGroup g;
};
static_assert(sizeof(ChainBoundsArgs) <= 4096, "the chain's argument block travels by value in the kernel arguments");

template <class Model, int E>
__global__ __launch_bounds__(kBlock) void chain_bounds_lower_kernel(ChainBoundsArgs k, int nblk)
{
    extern __shared__ uint4 sh_bt[];
    __shared__ double red[kNQ * kRedStride];
    chain_bounds_lower_body<Model, E>(k.d.v, k.g, Model{k.d}, nblk, sh_bt, red);
}

template <class Model, int E>
__global__ __launch_bounds__(kBlock) void chain_bounds_inner_kernel(ChainBoundsArgs k, int64_t i0, int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    chain_bounds_inner_body<Model, E>(k.d.v, k.g, Model{k.d}, i0, ni, sh_bt);
}

BoundsArgs chain_bounds_entry_args(const BoundsArgs& a, const ChainBoundsEntry& e)
{
    BoundsArgs b = a;
    b.K = e.K; b.invK = e.invK; b.is_put = e.is_put;
    b.betas = e.betas; b.tab = e.tab;
    b.q = e.q; b.samples = e.samples; b.steps = e.steps; b.part = e.part;
    return b;
}

namespace {
// the launches' common checks: a listed model, a group the kernels and their LDS have room for
bool chain_bounds_ok(int mo, const BoundsArgs& a, const ChainBoundsGroup& g)
{
    return mo >= 0 && mo <= 2 && g.E >= 1 && g.E <= chain_bounds_group_max(a.N);
}

// f(model constant, entries constant) for the group's model and length
template <class F>
void for_chain_bounds(int mo, int E, F&& f)
{
    for_int<0, 1, 2>(mo, [&](auto model) {
        for_int<1, 2, 3, 4, 5, 6, 7, 8>(E, [&](auto entries) { f(model, entries); });
    });
}
static_assert(kChainBoundsMax == 8, "for_chain_bounds lists the group lengths 1 .. kChainBoundsMax");
}  // namespace

hipError_t chain_bounds_lower(hipStream_t st, const BoundsArgs& a, const DiffusionLaw& l, const ChainBoundsGroup& g,
                              double* const* result)
{
    const int mo = diffusion_model(l);
    if (!chain_bounds_ok(mo, a, g)) return hipErrorInvalidValue;
    const ChainBoundsArgs k{diffusion_args(a, l), g};
    const int nblk = (int)bounds_lower_blocks(a);
    for_chain_bounds(mo, g.E, [&](auto model, auto entries) {
        constexpr int E = decltype(entries)::value;
        hipLaunchKernelGGL((chain_bounds_lower_kernel<DiffusionModel<decltype(model)::value>, E>), dim3(nblk), dim3(kBlock),
                           bounds_table_lds(a.N) * E, st, k, nblk);
    });
    for (int e = 0; e < g.E; ++e) {
        const hipError_t err = lsm_finalize(st, g.e[e].part, nullptr, result[e], nblk, 0);
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

hipError_t chain_bounds_inner(hipStream_t st, const BoundsArgs& a, const DiffusionLaw& l, const ChainBoundsGroup& g, int64_t i0,
                              int64_t ni)
{
    const int mo = diffusion_model(l);
    if (!chain_bounds_ok(mo, a, g) || i0 < 0 || ni < 1 || i0 + ni > a.n_outer) return hipErrorInvalidValue;
    const ChainBoundsArgs k{diffusion_args(a, l), g};
    for_chain_bounds(mo, g.E, [&](auto model, auto entries) {
        constexpr int E = decltype(entries)::value;
        hipLaunchKernelGGL((chain_bounds_inner_kernel<DiffusionModel<decltype(model)::value>, E>), dim3(bounds_inner_grid(ni * a.N)),
                           dim3(kBlock), bounds_table_lds(a.N) * E, st, k, i0, ni);
    });
    return hipGetLastError();
}

}  // namespace omc
