// omc_bounds_check_dev.h -- the bound kernels' bodies with Broadie-Cao's sub-optimality checking (option
// "bounds_suboptimality" = m >= 1; the rule is include/omc.h's): inner simulations run only at the
// (outer path, date) items at which exercise is not known to be sub-optimal, and the walk visits only those dates.
//
// The rule.  With s = So[t][i] (float32), x = (double)s, phi(x) = K - x (put) or x - K (call), item (i, t), 0 <= t < N, is
// KEPT iff one of
//     t == 0;    stop(s, t) (bd_stop: the exercise tables, the float64 rule on irregular dates);
//     m == 1 and phi(x) > 0;
//     m == 2 and phi(x) > E(x, t), E the Black-Scholes value of omc_bounds_cv_dev.h formed in float64 from its table of
//                per-date constants -- evaluated as not (phi(x) <= E(x, t)), so that a NaN keeps the item.
// The expiry t = N is always a date of the walk.  Paths, Philox coordinates, lane assignment, stopping rule, tables and the
// fixed-order sums are those of omc_bounds_dev.h / omc_bounds_cv_dev.h: Q^ of a kept item has the unchecked call's bits, a
// skipped item's entry stays the 0.0 the flow cleared it to, and the step count is the kept items'.
//
//   mark      one thread per (t, i): the keep mask [N][n_outer], one byte per item, date-major as So, and how many items
//             of every date each inner-launch block [b blk, (b + 1) blk) keeps (integer atomic sums, one per wave where a
//             wave lies within one date and block).
//   compact   per inner-launch block [i0, i0 + ni): the kept item numbers q = t * ni + (i - i0) as uint32, ascending (so
//             date-major, the longest items first), and their count -- a workgroup per date, which starts at the sum of
//             the earlier dates' counts and scans its 1024 x 8 items per round.  No host synchronisation: the sweeps read
//             the count from memory.
//   inner     bounds_inner_body / bounds_inner_cv_body<G, false, Park> with the item taken from the list; everything after
//             "which item" is theirs, line for line, and a change to either must be made here too.
//   walk      bd_sample's recursion over the kept dates and N.  Between two kept dates the policy continues, so the dense
//             walk's increments telescope to L_k - Q^_l; with every item kept the operations are bd_sample's, spelled as
//             omc_bounds2_dev.h spells them, and the bits are the dense walk's.
#pragma once
#include "omc_bounds_cv_dev.h"
#include "omc_bounds_dev.h"

namespace omc {

constexpr int kCheckBlock = 1024;  // the compaction's workgroup (one per date)
constexpr int kCheckPer = 8;       // items per thread and scan

// E(x, d) for d < N, undiscounted: bcv_euro's value without D[d]
__device__ __forceinline__ double bck_euro(double x, int d, double K, int is_put, const double* __restrict__ cv)
{
    const double* row = cv + (size_t)d * 4;
    const double mu = row[0], sq = row[1], Kd = row[2];
    const double d1 = (log(x / K) + mu) / sq;
    const double d2 = d1 - sq;
    const double sg = is_put ? -1.0 : 1.0;
    return sg * (x * bcv_phi(sg * d1) - Kd * bcv_phi(sg * d2));
}

// ------------------------------------------------------------------ mark
__device__ __forceinline__ void bounds_check_mark_body(const BoundsArgs& a, const BoundsCheck& k, const double* __restrict__ cv)
{
    const int64_t n = (int64_t)a.N * a.n_outer;
    for (int64_t at = (int64_t)blockIdx.x * kBlock + threadIdx.x; at < n; at += (int64_t)gridDim.x * kBlock) {
        const int t = (int)(at / a.n_outer);
        const int64_t i = at - (int64_t)t * a.n_outer;
        bool keep = t == 0;
        if (!keep) {
            const float s = a.So[at];
            const uint4 iv = *reinterpret_cast<const uint4*>(a.tab + (size_t)t * 8);
            keep = bd_stop(s, t, iv, a);
            if (!keep) {
                const double phi = payoff_d(s, a.K, a.is_put);
                if (k.mode == 1) keep = phi > 0.0;
                else keep = !(phi <= bck_euro((double)s, t, a.K, a.is_put, cv));  // phi > E, or a NaN
            }
        }
        k.keep[at] = keep ? 1 : 0;
        // the kept items of (launch block, date): one atomic per wave where its lanes share the slot, else one per kept item
        const uint32_t slot = (uint32_t)((i / k.blk) * a.N + t);  // < n_outer N < 2^32
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot);
        const uint64_t live = __builtin_amdgcn_ballot_w64(true), kept = __builtin_amdgcn_ballot_w64(keep);
        if (__builtin_amdgcn_ballot_w64(slot != first) == 0) {
            const bool lead = __builtin_amdgcn_mbcnt_hi((uint32_t)(live >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)live, 0)) == 0;
            if (lead && kept) atomicAdd(k.per_date + first, (uint32_t)__popcll(kept));
        } else if (keep) {
            atomicAdd(k.per_date + slot, 1u);
        }
    }
}

// ------------------------------------------------------------------ compaction
// workgroup t (kCheckBlock threads) lists date t; thread j of a round takes kCheckPer consecutive outer paths.  i0 is a
// multiple of k.blk and ni <= k.blk (the launcher checks).  sh_w [kCheckBlock / 64]
__device__ __forceinline__ void bounds_check_compact_body(const BoundsArgs& a, const BoundsCheck& k, int64_t i0, int64_t ni,
                                                          uint32_t* sh_w)
{
    const int t = (int)blockIdx.x;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    constexpr int kWaves = kCheckBlock / 64;
    const uint32_t* per = k.per_date + (size_t)(i0 / k.blk) * a.N;
    uint32_t base = 0;  // kept items before this round: the earlier dates', then this date's; the same in every thread
    for (int d = 0; d < t; ++d) base += per[d];
    const unsigned char* row = k.keep + (size_t)t * a.n_outer + i0;
    for (int64_t r0 = 0; r0 < ni; r0 += (int64_t)kCheckBlock * kCheckPer) {
        const int64_t j0 = r0 + (int64_t)threadIdx.x * kCheckPer;
        const int64_t first = (int64_t)t * ni + j0;  // the item number of j0
        uint32_t bits = 0;
#pragma unroll
        for (int u = 0; u < kCheckPer; ++u)
            if (j0 + u < ni) bits |= (row[j0 + u] ? 1u : 0u) << u;
        const uint32_t cnt = (uint32_t)__popc(bits);
        uint32_t incl = cnt;  // inclusive scan over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, off, 64);
            if (lane >= off) incl += v;
        }
        if (lane == 63) sh_w[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const uint32_t c = sh_w[w];
            before += w < wave ? c : 0u;
            total += c;
        }
        uint32_t at = base + before + incl - cnt;
#pragma unroll
        for (int u = 0; u < kCheckPer; ++u)
            if ((bits >> u) & 1u) k.list[at++] = (uint32_t)(first + u);
        base += total;
        __syncthreads();  // sh_w is written again
    }
    if (t == a.N - 1 && threadIdx.x == 0) *k.count = base;  // the last date's workgroup ends at the total
}

// ------------------------------------------------------------------ inner simulations (bounds_inner_body)
// a wave owns one entry of the list at a time, a lane one antithetic inner pair; sh_bt [N+1] dynamic LDS
template <class Model>
__device__ __forceinline__ void bounds_check_inner_body(const BoundsArgs& a, const BoundsCheck& ck, const Model& m, int64_t i0,
                                                        int64_t ni, uint4* sh_bt)
{
    bd_load_tables(a, sh_bt);
    const int N = a.N;
    const int lane = (int)(threadIdx.x & 63);
    const int64_t H = a.half_inner;
    const int64_t n_kept = (int64_t)*ck.count;  // <= ni * N, the list's room
    const int64_t nwaves = (int64_t)gridDim.x * (kBlock / 64);
    unsigned long long steps = 0;
    for (int64_t e = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); e < n_kept; e += nwaves) {
        const int64_t item = (int64_t)ck.list[e];
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
                        if constexpr (bd_model_stops<Model>::value) bd_mark_stops(m, s, d, sh_bt[d], a, xa, xb, da, db);
                        else bd_mark(m.index_a(s), m.index_b(s), d, sh_bt[d], a, xa, xb, da, db);
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

// ------------------------------------------------------------------ controlled inner simulations (bounds_inner_cv_body)
// a wave takes 64 / G consecutive entries of the list at a time, group g of its lanes the g-th of them
template <int G, int Park, class Model>
__device__ __forceinline__ void bounds_check_inner_cv_body(const BoundsCvArgs& c, const BoundsCheck& ck, const Model& m,
                                                           int64_t i0, int64_t ni, uint4* sh_bt)
{
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "a lane group is 8, 16, 32 or 64 lanes");
    const BoundsArgs& a = c.b;
    bd_load_tables(a, sh_bt);
    const int N = a.N;
    constexpr int kGroups = 64 / G;
    const int lane = (int)(threadIdx.x & 63);
    const int grp = lane / G, gl = lane & (G - 1);
    const uint64_t gmask = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull) << (grp * G);
    const int64_t H = a.half_inner;
    const int64_t n_kept = (int64_t)*ck.count;  // <= ni * N, the list's room
    const int64_t stride = (int64_t)gridDim.x * (kBlock / 64) * kGroups;
    unsigned long long steps = 0;
    for (int64_t base = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * kGroups; base < n_kept; base += stride) {
        const bool has = base + grp < n_kept;                          // a wave's last entries may leave groups without one
        const int64_t item = (int64_t)ck.list[has ? base + grp : base];  // (those read the first group's start, simulate nothing)
        const int t = (int)(item / ni);
        const int64_t i = i0 + (item - (int64_t)t * ni);
        const float s0 = m.inner_start(t, i);
        const uint64_t gbase = ((uint64_t)i * (uint64_t)(N + 1) + (uint64_t)t) * (uint64_t)H;
        int64_t j = gl, next = G;  // this lane's pair; the item's first unstarted pair
        bool act = has && j < H;
        typename Model::Spots s;
        m.reset(s, s0);
        float xa = 0.0f, xb = 0.0f;
        int k = 0, da = 0, db = 0;  // steps taken by the pair; stop dates of its partners (0 while live)
        double acc = 0.0;
        // Every pair ends (bd_stop is true at d >= N), and a lane that waits (Park) is evaluated at the latest when no lane of
        // the wave is live: every iteration steps a pair or refills a lane.
        while (__builtin_amdgcn_ballot_w64(act)) {
            if (act && (da == 0 || db == 0)) {
                typename Model::Normals z;
                m.draw(gbase + (uint64_t)j, (uint32_t)(k >> 2), a.stream_inner, z);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (da == 0 || db == 0) {
                        ++k;
                        m.step(s, z, u);
                        bd_mark(m.index_a(s), m.index_b(s), t + k, sh_bt[t + k], a, xa, xb, da, db);
                    }
                }
            }
            const bool done = act && da != 0 && db != 0;
            bool refill = done;
            if (Park) {
                const bool need = done && (da < N || db < N);
                const int waiting = __popcll(__builtin_amdgcn_ballot_w64(need));
                const bool live = __builtin_amdgcn_ballot_w64(act && !done) != 0;
                refill = done && (!need || waiting >= Park || !live);
            }
            const uint64_t fin = __builtin_amdgcn_ballot_w64(refill) & gmask;
            if (refill) {
                acc += bcv_pair(xa, da, xb, db, c);
                steps += (unsigned long long)(da - t) + (unsigned long long)(db - t);
                // the group's finished lanes take the item's next pairs in lane order (mbcnt: finished lanes below this one)
                j = next + (int64_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(fin >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fin, 0));
                act = j < H;
                m.reset(s, s0);
                k = da = db = 0;
            }
            next += __popcll(fin);
        }
        double q = acc;
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) q += __shfl_xor(q, off, 64);
        if (has && gl == 0) a.q[(size_t)i * N + t] = bcv_euro(s0, t, c) + q / (double)(2 * H);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) steps += __shfl_xor(steps, off, 64);
    if (lane == 0 && steps) atomicAdd(a.steps, steps);
}

// ------------------------------------------------------------------ outer walk
// M = 0, lq = Q^_0; at the kept dates t and at N: L = stop ? Z_t : Q^_t (Q^_N = 0), M = M + L - lq, candidate Z_t - M,
// lq = Q^_t.  Z - M as bounds_walk_kernel computes it (there the compiler contracts the product of Z into the subtraction),
// spelled out with nothing else contracted, as omc_bounds2_dev.h's walk does.
__device__ __forceinline__ double bd_check_sample(const BoundsArgs& a, const BoundsCheck& k, int64_t i)
{
#pragma clang fp contract(off)
    const int N = a.N;
    const double* q = a.q + (size_t)i * N;
    double M = 0.0, qprev = q[0], best = -__builtin_huge_val();
    for (int t = 1; t <= N; ++t) {
        if (t < N && !k.keep[(size_t)t * a.n_outer + i]) continue;
        const float s = a.So[(size_t)t * a.n_outer + i];
        double pay = payoff_d(s, a.K, a.is_put);
        pay = pay > 0.0 ? pay : 0.0;
        const double Dt = a.D[t], Z = Dt * pay;  // bd_value
        const uint4 iv = *reinterpret_cast<const uint4*>(a.tab + (size_t)t * 8);
        const double qt = t < N ? q[t] : 0.0;
        const double L = bd_stop(s, t, iv, a) ? Z : qt;
        M = M + L - qprev;
        const double x = fma(Dt, pay, -M);
        best = x > best ? x : best;
        qprev = qt;
    }
    return best;
}

// one thread per outer pair; red [kNQ * kRedStride]
__device__ __forceinline__ void bounds_check_walk_body(const BoundsArgs& a, const BoundsCheck& k, int nblk, double* red)
{
    double acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0;
    const int64_t P = a.n_outer / 2;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < P; p += (int64_t)nblk * kBlock) {
        const double xa = bd_check_sample(a, k, p), xb = bd_check_sample(a, k, p + P);
        a.samples[p] = xa;
        a.samples[p + P] = xb;
        const double m = 0.5 * (xa + xb);
        acc[0] += m;
        acc[1] += m * m;
    }
    const double s = block_reduce8(acc, red);
    if (threadIdx.x < 64 && (threadIdx.x & 7) == 0) a.part[(size_t)(threadIdx.x >> 3) * kPStride + blockIdx.x] = s;
}

}  // namespace omc
