// omc_bounds.h -- host interface of the Andersen-Broadie bound kernels (omc_bounds.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace omc {

// Sums the two sweeps leave in their result buffers (8 doubles each, float64, fixed order; lsm_finalize's slots 0..3):
//   lower:  0 sum of pair means of Z at tau_1   1 their squares   2 paths stopped before N   3 -
//   upper:  0 sum of pair means of the samples  1 their squares   2 -                        3 -
struct BoundsArgs {
    int N, is_put;
    double K, invK;
    float s0, a, b;           // the generator's float32 start value and step constants (gbm_step_constants)
    uint32_t k0, k1;          // Philox key = seed
    const double* D;          // [N+1] exp(-r dt t): Z_t = D[t] max(phi(S_t), 0)
    const double* betas;      // [N+1][4] the policy (float64 fallback on irregular steps)
    const uint32_t* tab;      // [N+1][8] exercise tables of lsm_crit_build_body (stored-path kind in slots 0..3)
    // lower bound
    int64_t n_lower;
    uint32_t stream_lower;
    // upper bound
    const float* So;          // [N+1][n_outer] outer paths (omc_gbm_paths_f32 at stream_outer)
    int64_t n_outer, half_inner;
    uint32_t stream_inner;
    double* q;                // [n_outer][N] Q^_t
    double* samples;          // [n_outer]
    unsigned long long* steps;  // inner path steps (integer sum)
    double* part;             // [8][kPStride] per-workgroup partials
};

int64_t bounds_lower_blocks(const BoundsArgs& a);
// the grid of every inner sweep: four item waves per workgroup (the control variate's lane groups: per_block items), at
// most 2048 workgroups
inline unsigned bounds_inner_grid(int64_t items, int64_t per_block = 4)
{
    const int64_t g = (items + per_block - 1) / per_block;
    return (unsigned)(g > 2048 ? 2048 : g);
}
// dynamic LDS of the sweeps that decide on one float32 index: the exercise tables, a uint4 per date
inline size_t bounds_table_lds(int N) { return sizeof(uint4) * (size_t)(N + 1); }
hipError_t bounds_lower(hipStream_t st, const BoundsArgs& a, double* result);
// Q^_t[i] for outer paths [i0, i0 + ni) and t = 0..N-1
hipError_t bounds_inner(hipStream_t st, const BoundsArgs& a, int64_t i0, int64_t ni);
int64_t bounds_walk_blocks(const BoundsArgs& a);
hipError_t bounds_walk(hipStream_t st, const BoundsArgs& a, double* result);

// An exercise schedule on the grid of N steps (option "bounds_exercise_every" = k >= 2): the dates
// tau_j = tau1 + (j - 1) k, j = 1 .. J, with tau_J = N, and tau_0 = 0.  bounds_schedule(N, k) builds it; the launchers below
// refuse (hipErrorInvalidValue) one that does not end at N, on which the inner sweep's termination rests.
struct BoundsSched {
    int k, J, tau1;
};
BoundsSched bounds_schedule(int N, int64_t every);  // every >= 2; k = min(every, N), J = (N - 1) / k + 1
bool bounds_schedule_ok(const BoundsSched& sc, int N);
// Q^ at the dates tau_0 .. tau_{J-1} for outer paths [i0, i0 + ni): column tau_j of a.q (the other columns are not written)
hipError_t bounds_sched_inner(hipStream_t st, const BoundsArgs& a, const BoundsSched& sc, int64_t i0, int64_t ni);
hipError_t bounds_sched_walk(hipStream_t st, const BoundsArgs& a, const BoundsSched& sc, double* result);
// rows 0, tau_1 .. tau_J of S [N+1][ld] to its rows 0 .. J, in place
hipError_t bounds_sched_gather(hipStream_t st, float* S, int64_t ld, const BoundsSched& sc);
// dst [N+1][4] <- the scheduled rows of src (gathered: src is [J+1][4], row j for date tau_j; else src is [N+1][4] and may be
// dst), zero rows elsewhere
hipError_t bounds_sched_policy(hipStream_t st, const double* src, double* dst, int N, const BoundsSched& sc, bool gathered);

// The Black-Scholes control variate of the GBM bounds (option "bounds_control_variate" = 1; DESIGN.md section 26,
// omc_bounds_cv_dev.h): BoundsArgs, the law's parameters in double and the table of E's per-date constants.
struct BoundsCvArgs {
    BoundsArgs b;
    double r, sigma, dt;  // dt = T / N
    double* cv;           // [N+1][4] (r + sigma^2 / 2) tau, sigma sqrt(tau), K exp(-r tau), tau = (N - d) dt
};
// how the controlled inner sweep is run (option "bounds_cv_form", for tests and measurement only; both forms compute the same
// Q^ up to the order of their sums)
enum { kCvFormDefault = 0, kCvFormWave = 1 };  // lane groups by n_inner; one item per wave (G = 64) whatever n_inner
int bounds_cv_group(int64_t half_inner, int form);  // G: the smallest of 8, 16, 32, 64 that is >= half_inner, at most 64
hipError_t bounds_cv_table(hipStream_t st, const BoundsCvArgs& c);
double bounds_cv_euro_host(double x, double K, double r, double sigma, double tau, bool is_put);  // E, on the host in double
hipError_t bounds_lower_cv(hipStream_t st, const BoundsCvArgs& c, double* result);
hipError_t bounds_inner_cv(hipStream_t st, const BoundsCvArgs& c, int form, int64_t i0, int64_t ni);
hipError_t bounds_sched_inner_cv(hipStream_t st, const BoundsCvArgs& c, const BoundsSched& sc, int form, int64_t i0, int64_t ni);

// Sub-optimality checking (option "bounds_suboptimality" = m >= 1; DESIGN.md section 27, omc_bounds_check_dev.h): inner
// simulations at the kept items only, the walk over the kept dates.
struct BoundsCheck {
    int mode;             // 1: kept where phi > 0, 2: kept where phi > E; t = 0 and the policy's stops are kept in both
    unsigned char* keep;  // [N][n_outer] the keep mask, date-major as So
    uint32_t* list;       // [ni N] of one inner launch: the kept item numbers t ni + (i - i0), ascending
    uint32_t* count;      // how many
    uint32_t* per_date;   // [ceil(n_outer / blk)][N] kept items of a date among the outer paths of an inner launch (zero
    int64_t blk;          // before the mark); blk: outer paths per inner launch, the launches start at its multiples
};
// the mask of every item; cv: BoundsCvArgs::cv, read in mode 2 alone
hipError_t bounds_check_mark(hipStream_t st, const BoundsArgs& a, const BoundsCheck& k, const double* cv);
hipError_t bounds_check_compact(hipStream_t st, const BoundsArgs& a, const BoundsCheck& k, int64_t i0, int64_t ni);
// Q^ at the listed items of outer paths [i0, i0 + ni); the other entries of a.q are not written
hipError_t bounds_check_inner(hipStream_t st, const BoundsArgs& a, const BoundsCheck& k, int64_t i0, int64_t ni);
hipError_t bounds_check_inner_cv(hipStream_t st, const BoundsCvArgs& c, const BoundsCheck& k, int form, int64_t i0, int64_t ni);
hipError_t bounds_check_walk(hipStream_t st, const BoundsArgs& a, const BoundsCheck& k, double* result);

// The diffusion of a one-asset law as the host knows it (Heston, jump-diffusion and dividend bounds: omc_bounds_law_dev.h);
// the launchers turn it into the generators' float32 constants (diffusion_args: gbm_step_constants or make_heston at the
// drift rate), so every spot is the generator's.
struct DiffusionLaw {
    int model, scheme;  // model 0 GBM, 1 Heston (scheme 0 reference clamp, 1 full truncation)
    double drift_rate;  // the rate of the paths (the discounts stay at r)
    double sigma, T, v0, kappa, theta, xi, rho;
    const float* Vo;    // Heston: [N+1][n_outer] the variance state of the outer paths
};
// the kernels' model number (0 GBM, 1 / 2 Heston scheme 0 / 1), or -1 for a law that has no kernels
inline int diffusion_model(const DiffusionLaw& l)
{
    if (l.model == 0) return 0;
    return l.model == 1 && (l.scheme == 0 || l.scheme == 1) ? l.scheme + 1 : -1;
}

}  // namespace omc
