// omc_dividend_bounds.h -- host interface of the dividend-law bound kernels and of the dividend generator that keeps the
// variance (omc_dividend_bounds.hip): GBM and Heston scheme 0 / 1 on a stock that pays discrete
// dividends.
#pragma once
#include <vector>

#include "omc_bounds.h"
#include "omc_dividend.h"

namespace omc {

// Where a path that starts at date t stands in the dividend table, in one word a lane keeps in a register:
//   bits 16 .. 27  ix, the first entry with step > t (the entry of step t itself is not applied again: the start spot is
//                  ex-dividend); n_steps <= 4094, so 12 bits hold it
//   bits 0 .. 15   the countdown: how many of the path's own steps are left until the one that has that dividend, or
//                  kDivNever behind the last entry -- a path takes at most 4094 steps, so it never runs out
// A step takes 1 off; the step after which the low half is 0 has the dividend, and adding (1 << 16) + gap moves on to the
// next entry (gap: the steps between the two, kDivNever behind the last).  (With the countdown in the high half the test is
// a subtract and a compare, one instruction fewer, but the register allocation comes out two registers higher and the
// scheduled GBM sweep falls from 7 waves per SIMD to 6: tried, not kept.)
using DivStart = uint32_t;
constexpr uint32_t kDivNever = 0x7000;
inline DivStart div_start(int ix, uint32_t countdown) { return ((uint32_t)ix << 16) | countdown; }

// The device tables of a call, composed on the host from omc_dividend_schedule's table mul / cash / has [N+1]:
//   tab          the entries with step > step_offset, in step order, their steps counted from step_offset, closed by the
//                entry {kDivNoStep, 1, 0}: the generator's table of a path that starts at date step_offset; an entry's
//                pad holds the gap to the next entry's step (kDivNever: there is none), which the generator does not read
//   first_after  [N+1], from the table at step_offset = 0 (null: not wanted)
inline void dividend_tables(int N, const float* mul, const float* cash, const int32_t* has, int step_offset,
                            std::vector<DivEntry>* tab, std::vector<DivStart>* first_after)
{
    tab->clear();
    for (int k = step_offset + 1; k <= N; ++k)
        if (has[k]) tab->push_back(DivEntry{k - step_offset, mul[k], cash[k], 0});
    const size_t n_ent = tab->size();
    tab->push_back(DivEntry{kDivNoStep, 1.0f, 0.0f, 0});
    for (size_t j = 0; j < n_ent; ++j)
        (*tab)[j].pad = j + 1 < n_ent ? (*tab)[j + 1].step - (*tab)[j].step : (int32_t)kDivNever;
    if (!first_after) return;
    first_after->resize((size_t)N + 1);
    size_t ix = 0;
    for (int t = 0; t <= N; ++t) {
        while (ix < n_ent && (*tab)[ix].step <= t) ++ix;
        (*first_after)[(size_t)t] = div_start((int)ix, ix < n_ent ? (uint32_t)((*tab)[ix].step - t) : kDivNever);
    }
}

// the law of a dividend bounds call as the host knows it: the diffusion at the drift rate r - q, so every spot is the
// dividend generator's, and the device tables
struct DividendBoundsLaw {
    DiffusionLaw d;
    const DivEntry* tab;    // device: the call's table at step_offset = 0
    const DivStart* first;  // device: [N+1]
};

// launch_dividend_paths' S (one pair per thread) with the variance state V [n_steps+1][ld] beside it, as
// launch_heston_paths_sv stores it; a.paths.model = 1, scheme 0 .. 3
hipError_t launch_dividend_paths_sv(hipStream_t st, const DividendGen& a, float* V);

// bounds_lower / bounds_inner / bounds_sched_inner / bounds_check_inner (omc_bounds.h) under the dividend law; a model or a
// scheme that has no kernels is hipErrorInvalidValue
hipError_t bounds_lower(hipStream_t st, const BoundsArgs& a, const DividendBoundsLaw& l, double* result);
hipError_t bounds_inner(hipStream_t st, const BoundsArgs& a, const DividendBoundsLaw& l, int64_t i0, int64_t ni);
hipError_t bounds_sched_inner(hipStream_t st, const BoundsArgs& a, const DividendBoundsLaw& l, const BoundsSched& sc, int64_t i0,
                              int64_t ni);
hipError_t bounds_check_inner(hipStream_t st, const BoundsArgs& a, const DividendBoundsLaw& l, const BoundsCheck& k, int64_t i0,
                              int64_t ni);

}  // namespace omc
