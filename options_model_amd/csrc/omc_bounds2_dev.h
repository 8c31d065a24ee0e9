// omc_bounds2_dev.h -- the bound kernels' bodies for a policy on TWO regressors (x, y), written once for every path law
// (DESIGN.md sections 18.1 and 21.2; the rule and the row layout are include/omc.h's): the float64 rule behind a
// wave-uniform branch, the policy rows in LDS, the lower sweep, the inner simulations, the outer walk and the sums of one
// date of the Longstaff-Schwartz fit.
//
// The sweeps are bounds_lower_body / bounds_inner_body (omc_bounds_dev.h) with a pair of values per partner in the place
// of one float32 and a 64-byte row of float64 coefficients in the place of a uint4 exercise table: the loops, the stop
// bookkeeping, the ballot + mbcnt refill, the xor-shuffle sum and the step count are theirs, line for line, and a change
// to either must be made here too.  The walk is bounds_walk_kernel's bd_sample with the product of Z spelled out.
//
// omc_runnerup_bounds.hip holds the same bodies restated for the basket generator (its regressors are the index and the
// runner-up, both scaled by 1/K).  Those kernels are NOT moved onto this header here: that is a refactor that needs its
// own bit-for-bit evidence (disassembly and result bits against its parent), a change of its own.  Until then a change
// to the bodies below must be made there too.
//
// A path law is a Model, which supplies omc_bounds_dev.h's
//   Start, Spots, Normals, lower_start(), inner_start(t, i), reset(spots, start), draw(pair, blk, stream, z),
//   step(spots, z, u)
// and, in the place of index_a / index_b,
//   xy_a(spots), xy_b(spots)     what the policy sees of either partner: the pair (x, y) of float32
//   xy_outer(t, i)               ... of outer path i at date t (the walk)
// The scale of the second regressor is Rule2's: u = fma(x, 1/K, -1), w = fma(y, inv_y, -1).
#pragma once
#include "omc_bounds_dev.h"
#include "omc_runnerup_bounds.h"  // kRunnerupCols, kRunnerupSlots, kRunnerupFitBlocks: the row and the sums are section 18's

namespace omc {

struct Pair2 {
    float x, y;  // the regressors of one path at one date; the payoff is phi(x)
};

struct Rule2 {
    double K, invK, inv_y;  // inv_y: 1 / the scale of y
    float thr;              // phi(x) > 0 as one float32 compare (itm_threshold)
    int is_put, N;
};
__device__ __forceinline__ Rule2 b2_rule(double K, double invK, double inv_y, int is_put, int N)
{
    return {K, invK, inv_y, itm_threshold(K, is_put), is_put, N};
}
__device__ __forceinline__ bool b2_itm(float x, const Rule2& r) { return r.is_put ? x < r.thr : x > r.thr; }

// the float64 rule of a date t in 1 .. N-1 with the date's row (c0 .. c5, n, 0)
__device__ __forceinline__ bool b2_exercises(Pair2 p, const double* row, const Rule2& r)
{
    const double imm = payoff_d(p.x, r.K, r.is_put);
    const double u = fma((double)p.x, r.invK, -1.0), w = fma((double)p.y, r.inv_y, -1.0);
    const double cont = fma(w, fma(w, row[4], fma(u, row[5], row[3])), fma(u, fma(u, row[2], row[1]), row[0]));
    return (row[6] > 0.5) & (imm > 0.0) & (imm > cont);
}

// the policy rows [N+1][8] -> LDS
__device__ __forceinline__ void b2_load_policy(const double* __restrict__ pol, int N, double* sh)
{
    for (int i = threadIdx.x; i < (N + 1) * kRunnerupCols; i += blockDim.x) sh[i] = pol[i];
    __syncthreads();
}

// bd_mark with the two-regressor stop: one step of both partners' stop bookkeeping at date d.  The in-the-money test
// comes first, one float32 compare; the float64 polynomial runs only when a live partner of some lane of the wave is in
// the money at a date before N (ballot: a scalar branch)
__device__ __forceinline__ void b2_mark(Pair2 pa, Pair2 pb, int d, const double* sh_pol, const Rule2& r, float& xa, float& xb,
                                        int& da, int& db)
{
    bool ea = da == 0, eb = db == 0;
    if (d < r.N) {
        ea = ea && b2_itm(pa.x, r);
        eb = eb && b2_itm(pb.x, r);
        if (__builtin_amdgcn_ballot_w64(ea || eb)) {
            const double* row = sh_pol + (size_t)d * kRunnerupCols;
            ea = ea && b2_exercises(pa, row, r);
            eb = eb && b2_exercises(pb, row, r);
        }
    }
    xa = ea ? pa.x : xa;
    da = ea ? d : da;
    xb = eb ? pb.x : xb;
    db = eb ? d : db;
}

// ------------------------------------------------------------------ lower bound (bounds_lower_body)
// one thread per antithetic pair of fresh paths; sh_pol [N+1][8] dynamic LDS, red [kNQ * kRedStride]
template <class Model>
__device__ __forceinline__ void bounds2_lower_body(const BoundsArgs& a, const Model& m, const double* __restrict__ pol,
                                                   double inv_y, int nblk, double* sh_pol, double* red)
{
    b2_load_policy(pol, a.N, sh_pol);
    const Rule2 rule = b2_rule(a.K, a.invK, inv_y, a.is_put, a.N);
    const int N = a.N;
    double acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0;
    const int64_t P = a.n_lower / 2;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < P; p += (int64_t)nblk * kBlock) {
        typename Model::Spots s;
        m.reset(s, m.lower_start());
        float xa = 0.0f, xb = 0.0f;  // the x each partner stopped at (written by the stop that sets da / db)
        int da = 0, db = 0;          // stop dates, 0 while live
        for (int blk = 0; 4 * blk < N && (da == 0 || db == 0); ++blk) {
            typename Model::Normals z;
            m.draw((uint64_t)p, (uint32_t)blk, a.stream_lower, z);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int d = 4 * blk + u + 1;
                if (d > N) break;
                m.step(s, z, u);
                b2_mark(m.xy_a(s), m.xy_b(s), d, sh_pol, rule, xa, xb, da, db);
            }
        }
        const double v = 0.5 * (bd_value(xa, da, a) + bd_value(xb, db, a));
        acc[0] += v;
        acc[1] += v * v;
        acc[2] += (da < N ? 1.0 : 0.0) + (db < N ? 1.0 : 0.0);
    }
    const double r = block_reduce8(acc, red);
    if (threadIdx.x < 64 && (threadIdx.x & 7) == 0) a.part[(size_t)(threadIdx.x >> 3) * kPStride + blockIdx.x] = r;
}

// ------------------------------------------------------------------ inner simulations (bounds_inner_body)
// items q = t * ni + (i - i0); a wave owns one item at a time, a lane one antithetic inner pair; sh_pol [N+1][8] dynamic LDS
template <class Model>
__device__ __forceinline__ void bounds2_inner_body(const BoundsArgs& a, const Model& m, const double* __restrict__ pol,
                                                   double inv_y, int64_t i0, int64_t ni, double* sh_pol)
{
    b2_load_policy(pol, a.N, sh_pol);
    const Rule2 rule = b2_rule(a.K, a.invK, inv_y, a.is_put, a.N);
    const int N = a.N;
    const int lane = (int)(threadIdx.x & 63);
    const int64_t H = a.half_inner;
    const int64_t n_items = ni * N;
    const int64_t nwaves = (int64_t)gridDim.x * (kBlock / 64);
    unsigned long long steps = 0;
    for (int64_t item = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); item < n_items; item += nwaves) {
        const int t = (int)(item / ni);
        const int64_t i = i0 + (item - (int64_t)t * ni);
        const typename Model::Start s0 = m.inner_start(t, i);
        const uint64_t gbase = ((uint64_t)i * (uint64_t)(N + 1) + (uint64_t)t) * (uint64_t)H;
        int64_t j = lane, next = 64;  // this lane's pair; the item's first unstarted pair
        bool act = j < H;
        typename Model::Spots s;
        m.reset(s, s0);
        float xa = 0.0f, xb = 0.0f;
        int k = 0, da = 0, db = 0;  // steps taken by the pair; stop dates of its partners (0 while live)
        double acc = 0.0;
        while (__builtin_amdgcn_ballot_w64(act)) {
            if (act) {
                typename Model::Normals z;
                m.draw(gbase + (uint64_t)j, (uint32_t)(k >> 2), a.stream_inner, z);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (da == 0 || db == 0) {
                        ++k;
                        const int d = t + k;
                        m.step(s, z, u);
                        b2_mark(m.xy_a(s), m.xy_b(s), d, sh_pol, rule, xa, xb, da, db);
                    }
                }
            }
            const bool done = act && da != 0 && db != 0;
            const uint64_t fin = __builtin_amdgcn_ballot_w64(done);
            if (done) {
                acc += bd_value(xa, da, a) + bd_value(xb, db, a);
                steps += (unsigned long long)(da - t) + (unsigned long long)(db - t);
                // the finished lanes take the next pairs in lane order (mbcnt: finished lanes below this one)
                j = next + (int64_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(fin >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fin, 0));
                act = j < H;
                m.reset(s, s0);
                k = da = db = 0;
            }
            next += __popcll(fin);
        }
        const double q = wave_sum_f64(acc);
        if (lane == 0) a.q[(size_t)i * N + t] = q / (double)(2 * H);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) steps += __shfl_xor(steps, off, 64);
    if (lane == 0 && steps) atomicAdd(a.steps, steps);
}

// ------------------------------------------------------------------ outer walk (bd_sample / bounds_walk_kernel)
// the rows come from global memory: every thread reads every date's row once per path
template <class Model>
__device__ __forceinline__ double b2_sample(const BoundsArgs& a, const Model& m, const double* __restrict__ pol,
                                            const Rule2& rule, int64_t i)
{
#pragma clang fp contract(off)
    const int N = a.N;
    const double* q = a.q + (size_t)i * N;
    double M = 0.0, qprev = q[0], best = -__builtin_huge_val();
    for (int t = 1; t <= N; ++t) {
        const Pair2 p = m.xy_outer(t, i);
        double pay = payoff_d(p.x, a.K, a.is_put);
        pay = pay > 0.0 ? pay : 0.0;
        const double Dt = a.D[t], Z = Dt * pay;  // bd_value
        const double qt = t < N ? q[t] : 0.0;
        const bool stop = t >= N || (b2_itm(p.x, rule) && b2_exercises(p, pol + (size_t)t * kRunnerupCols, rule));
        const double L = stop ? Z : qt;
        M = M + L - qprev;
        // Z - M as bounds_walk_kernel computes it: there the compiler contracts the product of Z into the subtraction.  Spelled
        // out (and nothing else contracted: the pragma above), so that equal decisions give the one-regressor walk's bits
        const double x = fma(Dt, pay, -M);
        best = x > best ? x : best;
        qprev = qt;
    }
    return best;
}

template <class Model>
__device__ __forceinline__ void bounds2_walk_body(const BoundsArgs& a, const Model& m, const double* __restrict__ pol,
                                                  double inv_y, int nblk, double* red)
{
    const Rule2 rule = b2_rule(a.K, a.invK, inv_y, a.is_put, a.N);
    double acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0;
    const int64_t P = a.n_outer / 2;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < P; p += (int64_t)nblk * kBlock) {
        const double xa = b2_sample(a, m, pol, rule, p), xb = b2_sample(a, m, pol, rule, p + P);
        a.samples[p] = xa;
        a.samples[p + P] = xb;
        const double mean = 0.5 * (xa + xb);
        acc[0] += mean;
        acc[1] += mean * mean;
    }
    const double s = block_reduce8(acc, red);
    if (threadIdx.x < 64 && (threadIdx.x & 7) == 0) a.part[(size_t)(threadIdx.x >> 3) * kPStride + blockIdx.x] = s;
}

// ------------------------------------------------------------------ the fit: the sums of one date
// Date t of classic Longstaff-Schwartz (semantics 1 of lsm_step_body) on kept matrices [N+1][ld] of the regressors, read
// through xy_at(row * ld + column).  Every path first applies the rule of date t+1, solved by the launch before this one,
// to its state (x_ex, tex) -- at t = N-1 the state starts at (x_N, N) --; the paths with phi(x_t) > 0 then add
// y = D[tex - t] max(phi(x_ex), 0) and f = (u, u^2, w, w^2, uw) to the 27 sums: per thread in column order, per workgroup
// by block_reduce8 in four groups of eight.  part [kRunnerupSlots][kRunnerupFitBlocks] is what runnerup_fit_solve reads.
struct Fit2 {
    int64_t ld, M;
    int N, is_put;
    double K, invK, inv_y;
    const double* D;  // [N+1] exp(-r dt k)
    float* x_ex;      // [M] x at the path's exercise date
    int32_t* tex;     // [M] that date
    double* part;     // [kRunnerupSlots][kRunnerupFitBlocks] per-workgroup partial sums of one date
    double* pol;      // [N+1][8]: rows 0 and N cleared, rows N-1 .. 1 fitted
};

template <class XYAt>
__device__ __forceinline__ void fit2_sums_body(const Fit2& f, const XYAt& xy_at, int t, int nblk, double* red)
{
    const Rule2 rule = b2_rule(f.K, f.invK, f.inv_y, f.is_put, f.N);
    const bool init = t == f.N - 1;
    double row[kRunnerupCols];
#pragma unroll
    for (int q = 0; q < kRunnerupCols; ++q) row[q] = init ? 0.0 : f.pol[(size_t)(t + 1) * kRunnerupCols + q];
    double acc[kRunnerupSlots];
#pragma unroll
    for (int q = 0; q < kRunnerupSlots; ++q) acc[q] = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < f.M; j += (int64_t)nblk * kBlock) {
        const Pair2 next = xy_at((size_t)(t + 1) * f.ld + j);
        float xe = next.x;
        int32_t te = t + 1;
        bool changed = true;
        if (!init) {
            changed = b2_itm(next.x, rule) && b2_exercises(next, row, rule);
            xe = changed ? next.x : f.x_ex[j];
            te = changed ? t + 1 : f.tex[j];
        }
        if (changed) {
            f.x_ex[j] = xe;
            f.tex[j] = te;
        }
        const Pair2 p = xy_at((size_t)t * f.ld + j);
        if (b2_itm(p.x, rule)) {
            double pay = payoff_d(xe, f.K, f.is_put);
            pay = pay > 0.0 ? pay : 0.0;
            const double y = f.D[te - t] * pay;
            const double u = fma((double)p.x, f.invK, -1.0), w = fma((double)p.y, f.inv_y, -1.0);
            const double ft[5] = {u, u * u, w, w * w, u * w};
            acc[0] += 1.0;
            int q = 6;
#pragma unroll
            for (int a = 0; a < 5; ++a) {
                acc[1 + a] += ft[a];
                acc[22 + a] += ft[a] * y;
#pragma unroll
                for (int b = a; b < 5; ++b) acc[q++] += ft[a] * ft[b];
            }
            acc[21] += y;
        }
    }
#pragma unroll
    for (int grp = 0; grp < kRunnerupSlots / 8; ++grp) {
        double a8[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) a8[q] = acc[8 * grp + q];
        const double r = block_reduce8(a8, red);
        if (threadIdx.x < 64 && (threadIdx.x & 7) == 0)
            f.part[(size_t)(8 * grp + (threadIdx.x >> 3)) * kRunnerupFitBlocks + blockIdx.x] = r;
        __syncthreads();  // `red` is used again
    }
}

}  // namespace omc
