// omc_greeks.hip -- pathwise Greeks of the two-pass (v3) polynomial-LSM estimator with the exercise policy FROZEN
// (DESIGN.md section 10).  One extra sweep over the path matrix the pricing already holds.
//
// Every stored spot of every model here is proportional to S0, so the scenario "S0 bumped by a factor lambda" is the
// stored path times lambda: no new paths.  Per path the sweep follows three CHAINS -- lambda = 1 (the base pricing,
// with pass 2's very expressions), 1 + h and 1 - h -- each deciding with the same frozen fits on spot lambda s_t and
// remembering its own (exercise spot, exercise step).  On folded storage (omc_lsm_dev.h) the partner of every stored
// column has three chains as well: six per column.  All Greek terms are formed once, after the sweep, from those pairs:
//   delta  D_k phi'(s) s / S0                          vega  D_k phi'(s) s (ln(s/S0) - (r + sigma^2/2) k dt) / sigma
//   rho    -(k-1) dt cf + D_k phi'(s) s k dt           theta -[-r (k-1) dt / T cf + D_k phi'(s) s (ln(s/S0) + (r - sigma^2/2) k dt) / 2T]
//   gamma  (delta+ - delta-) / (2 h S0), delta+- = D_k+- phi'(lambda+- s_k+-) s_k+- / S0
// with D_k = D[k-1] (valued at t = dt, as the pricing) and phi' = -1{imm > 0} (put) / +1{imm > 0} (call).
//
// One thread owns VEC columns and walks them backward until every chain has exercised; rows arrive in batches with
// the next batch requested before the current one is decided (walk_rows, as the folded pass 2).  Grid = one thread per VEC columns
// (no grid-stride loop: the 20 sums are live only after the sweep), per-workgroup partials in a fixed order, then one
// finalize launch: two identical calls return identical bits.
#include "omc_greeks_dev.h"

namespace omc {

template <int VEC, bool FOLD, int PUT>
__global__ __launch_bounds__(kBlock) void lsm_greeks_kernel(GreeksArgs a)
{
    greeks_body<VEC, FOLD, PUT>(a, GreeksGrid{});  // (the body: omc_greeks_dev.h)
}

__global__ __launch_bounds__(kBlock) void lsm_greeks_finalize_kernel(const double* __restrict__ part, int64_t nblk,
                                                                     const double* __restrict__ gmom, int N,
                                                                     double* __restrict__ result)
{
    greeks_finalize_body(part, nblk, gmom, N, result, blockIdx.x);
}

int greeks_vec(const GreeksArgs& a)
{
    return rows_aligned(2, a.cols, a.S, a.ld) ? 2 : 1;
}

int64_t greeks_blocks(const GreeksArgs& a)
{
    const int64_t per = (int64_t)kBlock * greeks_vec(a);
    return (a.cols + per - 1) / per;
}

hipError_t lsm_greeks(hipStream_t st, const GreeksArgs& a, hipEvent_t ev_begin, hipEvent_t ev_end)
{
    const int64_t nblk = greeks_blocks(a);
    const size_t dyn = sizeof(double) * 4 * (size_t)(a.N + 1);
    if (ev_begin) (void)hipEventRecord(ev_begin, st);
    for_int<2, 1>(greeks_vec(a), [&](auto vec) {
        for_flag(a.cK != nullptr, [&](auto fold) {
            for_put(a.is_put, [&](auto put) {
                constexpr int VEC = decltype(vec)::value, PUT = decltype(put)::value;
                hipLaunchKernelGGL((lsm_greeks_kernel<VEC, decltype(fold)::value, PUT>), dim3((unsigned)nblk), dim3(kBlock), dyn,
                                   st, a);
            });
        });
    });
    if (ev_end) (void)hipEventRecord(ev_end, st);
    hipLaunchKernelGGL(lsm_greeks_finalize_kernel, dim3(3), dim3(kBlock), 0, st, a.part, nblk, a.gmom, a.N, a.result);
    return hipGetLastError();
}

}  // namespace omc
