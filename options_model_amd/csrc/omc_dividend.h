// omc_dividend.h -- host interface of the dividend path generator (omc_dividend.hip): American options on a stock that
// pays discrete dividends, priced on the path matrix itself.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "omc_kernels.h"

namespace omc {

// One dividend step of the composed schedule: after the model's own step `step` the spot becomes
// max(fma(s, mul, -cash), 0).  The device table is sorted by step and closed by an entry with step = kDivNoStep.
struct DivEntry {
    int32_t step;
    float mul, cash;
    int32_t pad;
};
static_assert(sizeof(DivEntry) == 16, "one 16-byte uniform load per dividend step");
constexpr int32_t kDivNoStep = 0x7fffffff;

struct DividendGen {
    PathSpec paths;       // r is the DRIFT rate r - q; S = the matrix [N+1][ld], full storage
    const DivEntry* tab;  // device: the dividend steps in step order + the closing entry
};

// the generator: rows 0 .. N of both partners of every pair, ex-dividend spots on the dividend steps
hipError_t launch_dividend_paths(hipStream_t st, const DividendGen& a);

}  // namespace omc
