// omc_bounds.hip -- Andersen-Broadie price bounds of the Bermudan option on the pricing grid.
//
// Three sweeps, all with one frozen exercise policy (betas [N+1][4]) and GBM paths from the generator's own Philox
// counters and spot recurrence:
//   lower   one thread per antithetic pair of fresh paths, in registers: each partner stops at the FIRST date the rule
//           fires (or N) and contributes Z = exp(-r tau dt) max(phi, 0); pair means reduced per workgroup.
//   inner   the hot path: for every (outer path i, date t) item the mean Q^_t[i] of Z at tau_{t+1} over n_inner inner
//           paths started at the outer spot S_t[i].  A wave owns one item at a time; each lane simulates one antithetic
//           inner PAIR four steps per Philox block and, when both partners have stopped, takes the item's next
//           unstarted pair -- inner paths end anywhere between 1 and N - t steps, and only the item's tail is lost to
//           lanes without work.
//   walk    one thread per outer pair: L^, M^ and max_t (Z_t - M^_t) per outer path, pair means reduced per workgroup.
// Decisions: pass 2's float32 exercise tables (omc_crit.h, the stored-path kind) -- two unsigned compares on the spot's
// bits -- and, on the steps the table builder marks irregular, the float64 rule itself.  Both give the same decisions.
// Sums: float64, per lane in a fixed order, per wave / workgroup in a fixed tree, then lsm_finalize: identical calls
// return identical bits (the inner step count is an integer atomic sum, exact in any order).
// The lower and the inner sweep are bounds_lower_body / bounds_inner_body (omc_bounds_dev.h), which the multi-asset
// kernels share; this file supplies their path law, one GBM asset, and the walk.  It also instantiates the sweeps of an
// exercise schedule (omc_bounds_sched_dev.h, section 25) and those with the Black-Scholes control variate
// (omc_bounds_cv_dev.h, section 26), and the kernels of sub-optimality checking (omc_bounds_check_dev.h, section 27).
#include <cmath>

#include "omc_bounds_cv_dev.h"
#include "omc_bounds_law_dev.h"

namespace omc {

// the path law of one GBM asset (the Model of omc_bounds_dev.h): the generator's counters and spot recurrence; the
// policy sees the spot
struct GbmBoundsModel {
    using Start = float;
    struct Spots { float a, b; };
    using Normals = float[4];
    using Args = BoundsArgs;
    const BoundsArgs& a;
    static __device__ __forceinline__ const BoundsArgs& common(const Args& a) { return a; }
    __device__ __forceinline__ Start lower_start() const { return a.s0; }
    __device__ __forceinline__ Start inner_start(int t, int64_t i) const { return a.So[(size_t)t * a.n_outer + i]; }
    __device__ __forceinline__ void reset(Spots& s, Start s0) const { s.a = s.b = s0; }
    __device__ __forceinline__ void draw(uint64_t pair, uint32_t blk, uint32_t stream, Normals& z) const
    {
        normals4(pair, blk, stream, a.k0, a.k1, z);
    }
    __device__ __forceinline__ void step(Spots& s, const Normals& z, int u) const
    {
        s.a = s.a * fast_exp2(__builtin_fmaf(a.b, z[u], a.a));
        s.b = s.b * fast_exp2(__builtin_fmaf(-a.b, z[u], a.a));
    }
    __device__ __forceinline__ float index_a(const Spots& s) const { return s.a; }
    __device__ __forceinline__ float index_b(const Spots& s) const { return s.b; }
};
// its four sweeps are omc_bounds_law_dev.h's wrappers and launchers with the one Model, whatever the number
template <int>
using GbmSweepModel = GbmBoundsModel;

// ------------------------------------------------------------------ lower bound
int64_t bounds_lower_blocks(const BoundsArgs& a)
{
    const int64_t P = a.n_lower / 2;
    const int64_t b = (P + kBlock - 1) / kBlock;
    return b < kMaxLsmBlocks ? b : kMaxLsmBlocks;
}

hipError_t bounds_lower(hipStream_t st, const BoundsArgs& a, double* result)
{
    return launch_bounds_lower<GbmSweepModel, 0>(st, 0, a, a, result);
}

// ------------------------------------------------------------------ inner simulations
hipError_t bounds_inner(hipStream_t st, const BoundsArgs& a, int64_t i0, int64_t ni)
{
    return launch_bounds_inner<GbmSweepModel, 0>(st, 0, a, a, i0, ni);
}

// ------------------------------------------------------------------ outer walk
__device__ __forceinline__ double bd_sample(const BoundsArgs& a, int64_t i)
{
    const int N = a.N;
    const double* q = a.q + (size_t)i * N;
    double M = 0.0, qprev = q[0], best = -__builtin_huge_val();
    for (int t = 1; t <= N; ++t) {
        const float s = a.So[(size_t)t * a.n_outer + i];
        const double Z = bd_value(s, t, a);
        const uint4 iv = *reinterpret_cast<const uint4*>(a.tab + (size_t)t * 8);
        const double qt = t < N ? q[t] : 0.0;
        const double L = bd_stop(s, t, iv, a) ? Z : qt;
        M = M + L - qprev;
        const double x = Z - M;
        best = x > best ? x : best;
        qprev = qt;
    }
    return best;
}

__global__ __launch_bounds__(kBlock) void bounds_walk_kernel(BoundsArgs a, int nblk)
{
    __shared__ double red[kNQ * kRedStride];
    double acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0;
    const int64_t P = a.n_outer / 2;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < P; p += (int64_t)nblk * kBlock) {
        const double xa = bd_sample(a, p), xb = bd_sample(a, p + P);
        a.samples[p] = xa;
        a.samples[p + P] = xb;
        const double m = 0.5 * (xa + xb);
        acc[0] += m;
        acc[1] += m * m;
    }
    const double s = block_reduce8(acc, red);
    if (threadIdx.x < 64 && (threadIdx.x & 7) == 0) a.part[(size_t)(threadIdx.x >> 3) * kPStride + blockIdx.x] = s;
}

int64_t bounds_walk_blocks(const BoundsArgs& a)
{
    const int64_t b = (a.n_outer / 2 + kBlock - 1) / kBlock;
    return b < kMaxLsmBlocks ? b : kMaxLsmBlocks;
}

hipError_t bounds_walk(hipStream_t st, const BoundsArgs& a, double* result)
{
    const int nblk = (int)bounds_walk_blocks(a);
    hipLaunchKernelGGL(bounds_walk_kernel, dim3(nblk), dim3(kBlock), 0, st, a, nblk);
    return lsm_finalize(st, a.part, nullptr, result, nblk, 0);
}

// ------------------------------------------------------------------ an exercise schedule
// the sweeps of omc_bounds_sched_dev.h with the GBM path law, and what is the same under every law that decides on the spot:
// the walk over the scheduled dates, the gather of the fit's rows, the scatter of the policy
BoundsSched bounds_schedule(int N, int64_t every)
{
    BoundsSched sc;
    sc.k = every >= N ? N : (int)every;  // beyond N every schedule is the expiry alone
    sc.J = (N - 1) / sc.k + 1;
    sc.tau1 = N - (sc.J - 1) * sc.k;
    return sc;
}

bool bounds_schedule_ok(const BoundsSched& sc, int N)
{
    return sc.k >= 1 && sc.J >= 1 && sc.tau1 >= 1 && sc.tau1 <= sc.k && (int64_t)sc.tau1 + (int64_t)(sc.J - 1) * sc.k == N;
}

hipError_t bounds_sched_inner(hipStream_t st, const BoundsArgs& a, const BoundsSched& sc, int64_t i0, int64_t ni)
{
    return launch_bounds_sched_inner<GbmSweepModel, 0>(st, 0, a, a, sc, i0, ni);
}

__global__ __launch_bounds__(kBlock) void bounds_sched_walk_kernel(BoundsArgs a, BoundsSched sc, int nblk)
{
    __shared__ double red[kNQ * kRedStride];
    bounds_sched_walk_body(a, sc, nblk, red);
}

hipError_t bounds_sched_walk(hipStream_t st, const BoundsArgs& a, const BoundsSched& sc, double* result)
{
    if (!bounds_schedule_ok(sc, a.N)) return hipErrorInvalidValue;
    const int nblk = (int)bounds_walk_blocks(a);
    hipLaunchKernelGGL(bounds_sched_walk_kernel, dim3(nblk), dim3(kBlock), 0, st, a, sc, nblk);
    return lsm_finalize(st, a.part, nullptr, result, nblk, 0);
}

__global__ __launch_bounds__(kBlock) void bounds_sched_gather_kernel(float* S, int64_t ld, BoundsSched sc)
{
    bounds_sched_gather_body(S, ld, sc);
}

hipError_t bounds_sched_gather(hipStream_t st, float* S, int64_t ld, const BoundsSched& sc)
{
    if (ld <= 0) return hipSuccess;
    hipLaunchKernelGGL(bounds_sched_gather_kernel, dim3((unsigned)((ld + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, S, ld, sc);
    return hipGetLastError();
}

__global__ __launch_bounds__(kBlock) void bounds_sched_policy_kernel(const double* src, double* dst, int N, BoundsSched sc,
                                                                     int gathered)
{
    bounds_sched_policy_body(src, dst, N, sc, gathered);
}

hipError_t bounds_sched_policy(hipStream_t st, const double* src, double* dst, int N, const BoundsSched& sc, bool gathered)
{
    if (!bounds_schedule_ok(sc, N)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bounds_sched_policy_kernel, dim3((unsigned)((N + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, src,
                       dst, N, sc, gathered ? 1 : 0);
    return hipGetLastError();
}

// ------------------------------------------------------------------ the Black-Scholes control variate
// the bodies of omc_bounds_cv_dev.h with the GBM path law; no kernel above is touched
__global__ __launch_bounds__(kBlock) void bounds_cv_table_kernel(BoundsCvArgs c) { bounds_cv_table_body(c); }

hipError_t bounds_cv_table(hipStream_t st, const BoundsCvArgs& c)
{
    hipLaunchKernelGGL(bounds_cv_table_kernel, dim3((unsigned)((c.b.N + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, c);
    return hipGetLastError();
}

double bounds_cv_euro_host(double x, double K, double r, double sigma, double tau, bool is_put)
{
    const double sq = sigma * std::sqrt(tau);
    const double d1 = (std::log(x / K) + (r + 0.5 * sigma * sigma) * tau) / sq;
    const double d2 = d1 - sq;
    const double sg = is_put ? -1.0 : 1.0;
    const auto phi = [](double y) { return 0.5 * std::erfc(-y / 1.4142135623730951); };
    return sg * (x * phi(sg * d1) - K * std::exp(-r * tau) * phi(sg * d2));
}

__global__ __launch_bounds__(kBlock) void bounds_lower_cv_kernel(BoundsCvArgs c, int nblk)
{
    extern __shared__ uint4 sh_bt[];
    __shared__ double red[kNQ * kRedStride];
    bounds_lower_cv_body(c, GbmBoundsModel{c.b}, nblk, sh_bt, red);
}

hipError_t bounds_lower_cv(hipStream_t st, const BoundsCvArgs& c, double* result)
{
    const int nblk = (int)bounds_lower_blocks(c.b);
    hipLaunchKernelGGL(bounds_lower_cv_kernel, dim3(nblk), dim3(kBlock), bounds_table_lds(c.b.N), st, c, nblk);
    return lsm_finalize(st, c.b.part, nullptr, result, nblk, 0);
}

template <int G, bool Sched, int Park>
__global__ __launch_bounds__(kBlock) void bounds_inner_cv_kernel(BoundsCvArgs c, BoundsSched sc, int64_t i0, int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bounds_inner_cv_body<G, Sched, Park>(c, sc, GbmBoundsModel{c.b}, i0, ni, sh_bt);
}

// Park: n > 0 = a finished pair waits until n lanes of its wave wait; 0 = it is evaluated in the iteration it ends, the form
// that lost and is not instantiated (measured on the default call at n_inner 1024: 8 lanes 16.9 ms, 16 15.1, 32 14.2, 48 14.0,
// at the stop 21.5; DESIGN.md sections 6.4 and 26.4)
constexpr int kCvPark = 32;

int bounds_cv_group(int64_t half_inner, int form)
{
    if (form == kCvFormWave) return 64;  // tests and measurement: bounds_inner_body's shape whatever n_inner
    return half_inner <= 8 ? 8 : (half_inner <= 16 ? 16 : (half_inner <= 32 ? 32 : 64));
}

namespace {
template <int G, bool Sched, int Park>
hipError_t launch_inner_cv(hipStream_t st, const BoundsCvArgs& c, const BoundsSched& sc, int64_t i0, int64_t ni)
{
    const int64_t items = ni * (Sched ? sc.J : c.b.N);
    const int64_t per_block = (kBlock / 64) * (64 / G);
    const unsigned g = bounds_inner_grid(items, per_block);
    hipLaunchKernelGGL((bounds_inner_cv_kernel<G, Sched, Park>), dim3(g), dim3(kBlock),
                       bounds_table_lds(c.b.N), st, c, sc, i0, ni);
    return hipGetLastError();
}

template <bool Sched, int Park>
hipError_t launch_inner_cv_g(hipStream_t st, const BoundsCvArgs& c, const BoundsSched& sc, int G, int64_t i0, int64_t ni)
{
    switch (G) {
    case 8: return launch_inner_cv<8, Sched, Park>(st, c, sc, i0, ni);
    case 16: return launch_inner_cv<16, Sched, Park>(st, c, sc, i0, ni);
    case 32: return launch_inner_cv<32, Sched, Park>(st, c, sc, i0, ni);
    default: return launch_inner_cv<64, Sched, Park>(st, c, sc, i0, ni);
    }
}

template <bool Sched>
hipError_t launch_inner_cv_form(hipStream_t st, const BoundsCvArgs& c, const BoundsSched& sc, int form, int64_t i0, int64_t ni)
{
    const int G = bounds_cv_group(c.b.half_inner, form);
    return launch_inner_cv_g<Sched, kCvPark>(st, c, sc, G, i0, ni);
}
}  // namespace

hipError_t bounds_inner_cv(hipStream_t st, const BoundsCvArgs& c, int form, int64_t i0, int64_t ni)
{
    return launch_inner_cv_form<false>(st, c, BoundsSched{}, form, i0, ni);
}

hipError_t bounds_sched_inner_cv(hipStream_t st, const BoundsCvArgs& c, const BoundsSched& sc, int form, int64_t i0, int64_t ni)
{
    if (!bounds_schedule_ok(sc, c.b.N)) return hipErrorInvalidValue;
    return launch_inner_cv_form<true>(st, c, sc, form, i0, ni);
}

// ------------------------------------------------------------------ sub-optimality checking
// the bodies of omc_bounds_check_dev.h: the mark, the compaction and the walk of every law that decides on one float32 index,
// and the list-driven sweeps with the GBM path law; no kernel above is touched
__global__ __launch_bounds__(kBlock) void bounds_check_mark_kernel(BoundsArgs a, BoundsCheck k, const double* cv)
{
    bounds_check_mark_body(a, k, cv);
}

hipError_t bounds_check_mark(hipStream_t st, const BoundsArgs& a, const BoundsCheck& k, const double* cv)
{
    if ((k.mode != 1 && k.mode != 2) || (k.mode == 2 && !cv) || k.blk < 1) return hipErrorInvalidValue;
    int64_t g = ((int64_t)a.N * a.n_outer + kBlock - 1) / kBlock;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(bounds_check_mark_kernel, dim3((unsigned)g), dim3(kBlock), 0, st, a, k, cv);
    return hipGetLastError();
}

__global__ __launch_bounds__(kCheckBlock) void bounds_check_compact_kernel(BoundsArgs a, BoundsCheck k, int64_t i0, int64_t ni)
{
    __shared__ uint32_t sh_w[kCheckBlock / 64];
    bounds_check_compact_body(a, k, i0, ni, sh_w);
}

hipError_t bounds_check_compact(hipStream_t st, const BoundsArgs& a, const BoundsCheck& k, int64_t i0, int64_t ni)
{
    if (i0 < 0 || ni < 1 || i0 + ni > a.n_outer || (double)ni * (double)a.N >= 4294967296.0 || k.blk < 1 || i0 % k.blk != 0 ||
        ni > k.blk)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(bounds_check_compact_kernel, dim3((unsigned)a.N), dim3(kCheckBlock), 0, st, a, k, i0, ni);
    return hipGetLastError();
}

hipError_t bounds_check_inner(hipStream_t st, const BoundsArgs& a, const BoundsCheck& k, int64_t i0, int64_t ni)
{
    return launch_bounds_check_inner<GbmSweepModel, 0>(st, 0, a, a, k, i0, ni);
}

template <int G, int Park>
__global__ __launch_bounds__(kBlock) void bounds_check_inner_cv_kernel(BoundsCvArgs c, BoundsCheck k, int64_t i0, int64_t ni)
{
    extern __shared__ uint4 sh_bt[];
    bounds_check_inner_cv_body<G, Park>(c, k, GbmBoundsModel{c.b}, i0, ni, sh_bt);
}

namespace {
template <int G>
hipError_t launch_check_inner_cv(hipStream_t st, const BoundsCvArgs& c, const BoundsCheck& k, int64_t i0, int64_t ni)
{
    const int64_t items = ni * c.b.N;
    const int64_t per_block = (kBlock / 64) * (64 / G);
    const unsigned g = bounds_inner_grid(items, per_block);
    hipLaunchKernelGGL((bounds_check_inner_cv_kernel<G, kCvPark>), dim3(g), dim3(kBlock),
                       bounds_table_lds(c.b.N), st, c, k, i0, ni);
    return hipGetLastError();
}
}  // namespace

hipError_t bounds_check_inner_cv(hipStream_t st, const BoundsCvArgs& c, const BoundsCheck& k, int form, int64_t i0, int64_t ni)
{
    switch (bounds_cv_group(c.b.half_inner, form)) {  // G as the dense controlled sweep chooses it
    case 8: return launch_check_inner_cv<8>(st, c, k, i0, ni);
    case 16: return launch_check_inner_cv<16>(st, c, k, i0, ni);
    case 32: return launch_check_inner_cv<32>(st, c, k, i0, ni);
    default: return launch_check_inner_cv<64>(st, c, k, i0, ni);
    }
}

__global__ __launch_bounds__(kBlock) void bounds_check_walk_kernel(BoundsArgs a, BoundsCheck k, int nblk)
{
    __shared__ double red[kNQ * kRedStride];
    bounds_check_walk_body(a, k, nblk, red);
}

hipError_t bounds_check_walk(hipStream_t st, const BoundsArgs& a, const BoundsCheck& k, double* result)
{
    const int nblk = (int)bounds_walk_blocks(a);
    hipLaunchKernelGGL(bounds_check_walk_kernel, dim3(nblk), dim3(kBlock), 0, st, a, k, nblk);
    return lsm_finalize(st, a.part, nullptr, result, nblk, 0);
}

}  // namespace omc
