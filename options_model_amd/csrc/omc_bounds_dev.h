// omc_bounds_dev.h -- what the bound kernels of every path law share (omc_bounds.hip: one GBM asset; omc_basket_bounds.hip:
// D correlated GBM assets; DESIGN.md sections 12.2 and 17.2): the stopping rule from the exercise tables, the discounted
// payoff, the tables' LDS copy, the wave sum -- and the two sweeps that simulate fresh paths.
//
// bounds_lower_body and bounds_inner_body hold the loops, the stop bookkeeping, the refill and the sums.  A path law is a
// Model, which supplies
//   Start, Spots, Normals        the start spots of a pair, both partners' spots, one Philox block of normals (four steps)
//   lower_start()                the start of every lower pair
//   inner_start(t, i)            the start of the inner pairs of item (outer path i, date t): wave-uniform
//   reset(spots, start)          both partners at the start
//   draw(pair, blk, stream, z)   the normals of generator pair `pair`, block `blk`
//   step(spots, z, u)            both partners one step on, with step u of the block (the partner takes -z)
//   index_a(spots), index_b(spots)   what the policy sees of either partner: a float32 spot for the exercise tables
// and, only if it declares `static constexpr bool kStops = true` (a path may end for a reason of the law's own: a knock-out,
// omc_barrier_bounds.hip; the other laws leave it off and their kernels carry no trace of it),
//   stopped_a(spots, d), stopped_b(spots, d)   the partner stops at the date d being marked whatever the policy says, at its
//                                        index there
//   start_dead(start)                    wave-uniform: an item started here simulates nothing (scheduled sweep)
// and nothing else: the dates, the tables, the payoff, the discount and the outputs are BoundsArgs'.  Everything is inlined
// into the __global__ function that names the model, which also declares the LDS.
#pragma once
#include <type_traits>

#include "omc_bounds.h"
#include "omc_lsm_dev.h"

namespace omc {

// does a path at spot s stop at date d?  iv = the date's table (lo0, lo1, len0, len1); an irregular date decides with
// the float64 rule of omc_lsm_apply_frozen
__device__ __forceinline__ bool bd_stop(float s, int d, uint4 iv, const BoundsArgs& a)
{
    if (d >= a.N) return true;
    if (iv.x == kCritIrregular) return exercises(pay_stored(s, a.K, a.invK, a.is_put), fit_given(a.betas, d, a.N));
    return crit_in(iv, __float_as_uint(s));
}

__device__ __forceinline__ double bd_value(float s, int d, const BoundsArgs& a)
{
    const double p = payoff_d(s, a.K, a.is_put);
    return a.D[d] * (p > 0.0 ? p : 0.0);
}

// the stored-path tables [N+1][8] -> LDS [N+1][4]
__device__ __forceinline__ void bd_load_tables(const BoundsArgs& a, uint4* sh)
{
    for (int t = threadIdx.x; t <= a.N; t += blockDim.x) sh[t] = *reinterpret_cast<const uint4*>(a.tab + (size_t)t * 8);
    __syncthreads();
}

__device__ __forceinline__ double wave_sum_f64(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// one step of both partners' stop bookkeeping at date d: the FIRST date the rule fires (xa / xb: the index there)
__device__ __forceinline__ void bd_mark(float ia, float ib, int d, uint4 iv, const BoundsArgs& a, float& xa, float& xb, int& da,
                                        int& db)
{
    const bool ea = da == 0 && bd_stop(ia, d, iv, a);
    const bool eb = db == 0 && bd_stop(ib, d, iv, a);
    xa = ea ? ia : xa;
    da = ea ? d : da;
    xb = eb ? ib : xb;
    db = eb ? d : db;
}

// a Model that stops paths for a reason of its own says so at compile time (kStops); one that does not is marked by bd_mark
template <class Model, class = void>
struct bd_model_stops : std::false_type {};
template <class Model>
struct bd_model_stops<Model, std::enable_if_t<Model::kStops>> : std::true_type {};

// bd_mark for a Model with kStops: the law's own stop counts as the rule firing -- the stop date enters the step count and
// the stopped-before-N count as an exercise at that date would, the value is that of the index there.  The sweeps choose
// between the two with `if constexpr` at the call itself, so that for every other Model the call is the one it always was.
template <class Model, class Spots>
__device__ __forceinline__ void bd_mark_stops(const Model& m, const Spots& s, int d, uint4 iv, const BoundsArgs& a, float& xa,
                                              float& xb, int& da, int& db)
{
    const float ia = m.index_a(s), ib = m.index_b(s);
    const bool ea = da == 0 && (m.stopped_a(s, d) || bd_stop(ia, d, iv, a));
    const bool eb = db == 0 && (m.stopped_b(s, d) || bd_stop(ib, d, iv, a));
    xa = ea ? ia : xa;
    da = ea ? d : da;
    xb = eb ? ib : xb;
    db = eb ? d : db;
}

// ------------------------------------------------------------------ lower bound
// one thread per antithetic pair of fresh paths; sh_bt [N+1] dynamic LDS, red [kNQ * kRedStride]
template <class Model>
__device__ __forceinline__ void bounds_lower_body(const BoundsArgs& a, const Model& m, int nblk, uint4* sh_bt, double* red)
{
    bd_load_tables(a, sh_bt);
    const int N = a.N;
    double acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0;
    const int64_t P = a.n_lower / 2;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < P; p += (int64_t)nblk * kBlock) {
        typename Model::Spots s;
        m.reset(s, m.lower_start());
        float xa = 0.0f, xb = 0.0f;  // the index each partner stopped at (written by the stop that sets da / db)
        int da = 0, db = 0;          // stop dates, 0 while live
        for (int blk = 0; 4 * blk < N && (da == 0 || db == 0); ++blk) {
            typename Model::Normals z;
            m.draw((uint64_t)p, (uint32_t)blk, a.stream_lower, z);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int d = 4 * blk + u + 1;
                if (d > N) break;
                m.step(s, z, u);
                if constexpr (bd_model_stops<Model>::value) bd_mark_stops(m, s, d, sh_bt[d], a, xa, xb, da, db);
                else bd_mark(m.index_a(s), m.index_b(s), d, sh_bt[d], a, xa, xb, da, db);
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

// ------------------------------------------------------------------ inner simulations
// items q = t * ni + (i - i0): all outer paths of the earliest date first, so the longest items start first.  A wave owns
// one item at a time, a lane one antithetic inner pair; sh_bt [N+1] dynamic LDS
template <class Model>
__device__ __forceinline__ void bounds_inner_body(const BoundsArgs& a, const Model& m, int64_t i0, int64_t ni, uint4* sh_bt)
{
    bd_load_tables(a, sh_bt);
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

}  // namespace omc
