// omc_bounds_sched_dev.h -- the bound kernels' bodies for an exercise SCHEDULE (option "bounds_exercise_every" = k >= 2;
// DESIGN.md section 25): the game whose exercise dates are tau_j = N - (J - j) k, j = 1 .. J, on the fine grid of N steps.
// The paths are the fine grid's in every sweep -- the Model of omc_bounds_dev.h, its counters and its steps -- and only the
// dates at which a path may stop, and at which inner simulations start, are the schedule's.
//   inner   bounds_inner_body's shape (a wave per item, a lane per antithetic pair, refill by ballot + mbcnt) with items at
//           tau_0 = 0, tau_1 .. tau_{J-1} only, and the stop bookkeeping at the scheduled dates only: a lane counts its
//           steps down to its next date and between dates it only steps.
//   walk    bd_sample's recursion over the scheduled dates.
//   gather  rows 0, tau_1 .. tau_J of a path matrix to its rows 0 .. J (what the policy is fitted on), and the fitted or
//           given table to the full [N+1][4] one with zero rows off the schedule.
// The lower bound needs no kernel of its own: a zero row of the policy gives an empty exercise table, and bounds_lower_body
// stops only where a table is non-empty.
#pragma once
#include "omc_bounds_dev.h"

namespace omc {

// tau_j = tau1 + (j - 1) k for j = 1 .. J with tau_J = N, and tau_0 = 0: tau1 = N - (J - 1) k is in 1 .. k
__device__ __forceinline__ int bs_tau(const BoundsSched& sc, int j) { return j == 0 ? 0 : sc.tau1 + (j - 1) * sc.k; }

// ------------------------------------------------------------------ inner simulations
// items q = j0 * ni + (i - i0) with t = tau_j0, j0 = 0 .. J-1: all outer paths of the earliest date first.  The inner pairs
// of item (i, t) are the generator pairs the all-dates sweep gives that item, block by block from the item's start, so an
// inner path here is the inner path of bounds_inner_body at the same (i, t); sh_bt [N+1] dynamic LDS, a row per date of the
// grid as there (a copy of the J + 1 scheduled rows alone needs a row counter per lane beside the countdown, and that
// register is the one that takes the GBM kernel from 72 to 74 VGPRs and from 7 waves per SIMD to 6)
template <class Model>
__device__ __forceinline__ void bounds_sched_inner_body(const BoundsArgs& a, const BoundsSched& sc, const Model& m, int64_t i0,
                                                        int64_t ni, uint4* sh_bt)
{
    bd_load_tables(a, sh_bt);
    const int N = a.N;
    const int lane = (int)(threadIdx.x & 63);
    const int64_t H = a.half_inner;
    const int64_t n_items = ni * sc.J;
    const int64_t nwaves = (int64_t)gridDim.x * (kBlock / 64);
    unsigned long long steps = 0;
    for (int64_t item = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); item < n_items; item += nwaves) {
        const int j0 = (int)(item / ni);
        const int64_t i = i0 + (item - (int64_t)j0 * ni);
        const int t = bs_tau(sc, j0);
        const int gap0 = j0 == 0 ? sc.tau1 : sc.k;  // steps from t to the first date a path may stop at
        const typename Model::Start s0 = m.inner_start(t, i);
        const uint64_t gbase = ((uint64_t)i * (uint64_t)(N + 1) + (uint64_t)t) * (uint64_t)H;
        int64_t j = lane, next = 64;  // this lane's pair; the item's first unstarted pair
        bool act = j < H;
        if constexpr (bd_model_stops<Model>::value) act = act && !m.start_dead(s0);  // (an item dead at its start: Q^ = 0)
        typename Model::Spots s;
        m.reset(s, s0);
        float xa = 0.0f, xb = 0.0f;
        int k = 0, da = 0, db = 0;  // steps taken by the pair; stop dates of its partners (0 while live)
        int cd = gap0;              // steps to the pair's next scheduled date
        double acc = 0.0;
        // Every pair ends: tau_J = N is a scheduled date (the launcher refuses a schedule that does not end at N), the
        // countdown reaches it after N - t steps, and bd_stop is true at d >= N whatever the table holds -- so t + k <= N too.
        // Lanes of one wave sit at different steps after a refill, so the date test is each lane's own.
        while (__builtin_amdgcn_ballot_w64(act)) {
            if (act) {
                typename Model::Normals z;
                m.draw(gbase + (uint64_t)j, (uint32_t)(k >> 2), a.stream_inner, z);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (da == 0 || db == 0) {
                        ++k;
                        m.step(s, z, u);
                        if (--cd == 0) {
                            if constexpr (bd_model_stops<Model>::value) bd_mark_stops(m, s, t + k, sh_bt[t + k], a, xa, xb, da, db);
                            else bd_mark(m.index_a(s), m.index_b(s), t + k, sh_bt[t + k], a, xa, xb, da, db);
                            cd = sc.k;
                        }
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
                cd = gap0;
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

// ------------------------------------------------------------------ outer walk
// M_0 = 0, M_j = M_{j-1} + L_j - Q^_{j-1}, L_j = Z_{tau_j} where the policy exercises (and at j = J), else Q^_j; the sample
// is max_j (Z_{tau_j} - M_j).  bd_sample's order of operations: M + L - qprev.
__device__ __forceinline__ double bd_sched_sample(const BoundsArgs& a, const BoundsSched& sc, int64_t i)
{
    const int N = a.N;
    const double* q = a.q + (size_t)i * N;
    double M = 0.0, qprev = q[0], best = -__builtin_huge_val();
    int t = sc.tau1;
    for (int j = 1; j <= sc.J; ++j, t += sc.k) {
        const float s = a.So[(size_t)t * a.n_outer + i];
        const double Z = bd_value(s, t, a);
        const uint4 iv = *reinterpret_cast<const uint4*>(a.tab + (size_t)t * 8);
        const double qt = j < sc.J ? q[t] : 0.0;
        const double L = bd_stop(s, t, iv, a) ? Z : qt;
        M = M + L - qprev;
        const double x = Z - M;
        best = x > best ? x : best;
        qprev = qt;
    }
    return best;
}

// one thread per outer pair; red [kNQ * kRedStride]
__device__ __forceinline__ void bounds_sched_walk_body(const BoundsArgs& a, const BoundsSched& sc, int nblk, double* red)
{
    double acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0;
    const int64_t P = a.n_outer / 2;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < P; p += (int64_t)nblk * kBlock) {
        const double xa = bd_sched_sample(a, sc, p), xb = bd_sched_sample(a, sc, p + P);
        a.samples[p] = xa;
        a.samples[p + P] = xb;
        const double m = 0.5 * (xa + xb);
        acc[0] += m;
        acc[1] += m * m;
    }
    const double s = block_reduce8(acc, red);
    if (threadIdx.x < 64 && (threadIdx.x & 7) == 0) a.part[(size_t)(threadIdx.x >> 3) * kPStride + blockIdx.x] = s;
}

// ------------------------------------------------------------------ the fit's rows
// S [N+1][ld] -> rows 0 .. J hold rows 0, tau_1 .. tau_J, in place: a thread owns a column and goes up the dates, so row
// tau_j >= j is read before this thread writes it (as row tau_j of a later date)
__device__ __forceinline__ void bounds_sched_gather_body(float* S, int64_t ld, const BoundsSched& sc)
{
    const int64_t col = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (col >= ld) return;
    int t = sc.tau1;
    for (int j = 1; j <= sc.J; ++j, t += sc.k) S[(size_t)j * ld + col] = S[(size_t)t * ld + col];
}

// dst [N+1][4]: row tau_j = row j of src (gathered: a fit on the gathered matrix) or row tau_j of src (the caller's table,
// src may be dst); every other row, row 0 included, zero.  One thread per row.
__device__ __forceinline__ void bounds_sched_policy_body(const double* src, double* dst, int N, const BoundsSched& sc, int gathered)
{
    const int t = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (t > N) return;
    const bool on = t >= sc.tau1 && (t - sc.tau1) % sc.k == 0;
    const int row = on ? (gathered ? (t - sc.tau1) / sc.k + 1 : t) : 0;
    double v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = on ? src[(size_t)row * 4 + c] : 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) dst[(size_t)t * 4 + c] = v[c];
}

}  // namespace omc
