// omc_bounds_cv_dev.h -- the bound kernels' bodies with the Black-Scholes control variate (option "bounds_control_variate"
// = 1), one GBM asset.  Paths, Philox coordinates, stopping rule, exercise tables, walk and Z are those
// of omc_bounds_dev.h / omc_bounds_sched_dev.h; only what is averaged changes.  With E(x, d) the Black-Scholes value of the
// European option at spot x and time to expiry (N - d) dt, a partner stopped at index x and date d contributes
//     c = Z - D[d] E(x, d)   (d < N),      c = 0.0 exactly, nothing evaluated   (d = N)
// -- D_t E(S_t, t) is a martingale on the grid, so c has conditional mean zero less the early-exercise premium -- and
//   lower   sums the centred pair means (c_a + c_b) / 2; the host adds E0 = D[0] E(S0, 0)
//   inner   writes Q^_t[i] = D[t] E(S_t[i], t) + (sum of c) / n_inner
// The per-date constants of E are a table [N+1][4] of doubles beside the exercise tables (bounds_cv_table_body), read from
// global memory: a pair reads two rows when it ends, against its tens of LDS reads of the exercise tables while it runs.
//
// The inner sweep takes a LANE GROUP of G = 8, 16, 32 or 64 lanes per item (the smallest G >= n_inner / 2, at most 64), so a
// wave holds 64 / G items: with n_inner = 16 the shape of bounds_inner_body would use 8 lanes of 64.  A group keeps its own
// item, start state, refill (ballot + mbcnt masked to the group) and fixed-order sum; G = 64 is bounds_inner_body's shape.
// The Philox coordinates of an inner pair do not depend on G, the order of the float64 sums does.
// Where a finished pair's control is evaluated (float64 log and two erfc per partner, under whatever mask the finished lanes
// make): a finished lane waits until Park lanes of the wave wait or no lane is live, and they are evaluated together.  Pairs
// whose partners both reach the expiry contribute 0 and never wait.  Park = 0 evaluates in the iteration the pair ends; it
// lost the measurement of DESIGN.md section 26.4 and is not instantiated.
#pragma once
#include "omc_bounds_dev.h"
#include "omc_bounds_sched_dev.h"

namespace omc {

// row d of the table: (r + sigma^2 / 2) tau, sigma sqrt(tau), K exp(-r tau), tau = (N - d) dt.  One thread per date.
__device__ __forceinline__ void bounds_cv_table_body(const BoundsCvArgs& c)
{
    const int d = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (d > c.b.N) return;
    const double tau = (double)(c.b.N - d) * c.dt;
    double* row = c.cv + (size_t)d * 4;
    row[0] = (c.r + 0.5 * c.sigma * c.sigma) * tau;
    row[1] = c.sigma * sqrt(tau);
    row[2] = c.b.K * exp(-c.r * tau);
    row[3] = tau;
}

__device__ __forceinline__ double bcv_phi(double y) { return 0.5 * erfc(-y / 1.4142135623730951); }

// D[d] E((double)s, d) for d < N (row N of the table has sigma sqrt(tau) = 0 and is never read)
__device__ __forceinline__ double bcv_euro(float s, int d, const BoundsCvArgs& c)
{
    const double x = (double)s;
    const double* row = c.cv + (size_t)d * 4;
    const double mu = row[0], sq = row[1], Kd = row[2];
    const double d1 = (log(x / c.b.K) + mu) / sq;
    const double d2 = d1 - sq;
    const double sg = c.b.is_put ? -1.0 : 1.0;
    return c.b.D[d] * (sg * (x * bcv_phi(sg * d1) - Kd * bcv_phi(sg * d2)));
}

// c_a + c_b of a finished pair; one copy of the evaluation's code, run once per partner that stopped before N
__device__ __forceinline__ double bcv_pair(float xa, int da, float xb, int db, const BoundsCvArgs& c)
{
    double sum = 0.0;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
        const float s = h ? xb : xa;
        const int d = h ? db : da;
        if (d < c.b.N) sum += bd_value(s, d, c.b) - bcv_euro(s, d, c);
    }
    return sum;
}

// ------------------------------------------------------------------ lower bound
// bounds_lower_body's loop with the centred pair mean where it sums the pair mean of Z
template <class Model>
__device__ __forceinline__ void bounds_lower_cv_body(const BoundsCvArgs& c, const Model& m, int nblk, uint4* sh_bt, double* red)
{
    const BoundsArgs& a = c.b;
    bd_load_tables(a, sh_bt);
    const int N = a.N;
    double acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0;
    const int64_t P = a.n_lower / 2;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < P; p += (int64_t)nblk * kBlock) {
        typename Model::Spots s;
        m.reset(s, m.lower_start());
        float xa = 0.0f, xb = 0.0f;
        int da = 0, db = 0;
        for (int blk = 0; 4 * blk < N && (da == 0 || db == 0); ++blk) {
            typename Model::Normals z;
            m.draw((uint64_t)p, (uint32_t)blk, a.stream_lower, z);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int d = 4 * blk + u + 1;
                if (d > N) break;
                m.step(s, z, u);
                bd_mark(m.index_a(s), m.index_b(s), d, sh_bt[d], a, xa, xb, da, db);
            }
        }
        const double v = 0.5 * bcv_pair(xa, da, xb, db, c);
        acc[0] += v;
        acc[1] += v * v;
        acc[2] += (da < N ? 1.0 : 0.0) + (db < N ? 1.0 : 0.0);
    }
    const double r = block_reduce8(acc, red);
    if (threadIdx.x < 64 && (threadIdx.x & 7) == 0) a.part[(size_t)(threadIdx.x >> 3) * kPStride + blockIdx.x] = r;
}

// ------------------------------------------------------------------ inner simulations
// Items as bounds_inner_body (Sched = false: q = t * ni + (i - i0)) or bounds_sched_inner_body (Sched = true: q = j0 * ni +
// (i - i0), t = tau_j0) orders them.  A wave takes 64 / G consecutive items at a time, group g of its lanes the g-th of them,
// and goes on to its next 64 / G items when every group has finished; lane l of a group starts pair l of its item and the
// lanes that end take the item's next pairs in lane order.  sh_bt [N+1] dynamic LDS.
template <int G, bool Sched, int Park, class Model>
__device__ __forceinline__ void bounds_inner_cv_body(const BoundsCvArgs& c, const BoundsSched& sc, const Model& m, int64_t i0,
                                                     int64_t ni, uint4* sh_bt)
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
    const int64_t n_items = ni * (Sched ? sc.J : N);
    const int64_t stride = (int64_t)gridDim.x * (kBlock / 64) * kGroups;
    unsigned long long steps = 0;
    for (int64_t base = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * kGroups; base < n_items; base += stride) {
        const bool has = base + grp < n_items;          // a wave's last items may leave groups without one
        const int64_t item = has ? base + grp : base;   // (those read the first group's start and simulate nothing)
        const int j0 = (int)(item / ni);
        const int64_t i = i0 + (item - (int64_t)j0 * ni);
        const int t = Sched ? bs_tau(sc, j0) : j0;
        const int gap0 = Sched ? (j0 == 0 ? sc.tau1 : sc.k) : 1;  // steps from t to the first date a path may stop at
        const float s0 = m.inner_start(t, i);
        const uint64_t gbase = ((uint64_t)i * (uint64_t)(N + 1) + (uint64_t)t) * (uint64_t)H;
        int64_t j = gl, next = G;  // this lane's pair; the item's first unstarted pair
        bool act = has && j < H;
        typename Model::Spots s;
        m.reset(s, s0);
        float xa = 0.0f, xb = 0.0f;
        int k = 0, da = 0, db = 0;  // steps taken by the pair; stop dates of its partners (0 while live)
        int cd = gap0;              // Sched: steps to the pair's next scheduled date
        double acc = 0.0;
        // Every pair ends (bd_stop is true at d >= N; a schedule ends at N, which the launcher checks), and a lane that waits
        // (Park) is evaluated at the latest when no lane of the wave is live: every iteration steps a pair or refills a lane.
        while (__builtin_amdgcn_ballot_w64(act)) {
            if (act && (da == 0 || db == 0)) {
                typename Model::Normals z;
                m.draw(gbase + (uint64_t)j, (uint32_t)(k >> 2), a.stream_inner, z);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (da == 0 || db == 0) {
                        ++k;
                        m.step(s, z, u);
                        if (!Sched || --cd == 0) {
                            bd_mark(m.index_a(s), m.index_b(s), t + k, sh_bt[t + k], a, xa, xb, da, db);
                            if (Sched) cd = sc.k;
                        }
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
                cd = gap0;
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

}  // namespace omc
