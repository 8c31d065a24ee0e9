// omc_chain_bounds_dev.h -- the two sweeps of omc_bounds_dev.h that simulate fresh paths, with E frozen policies riding on
// one simulation of every path (omc_chain_bounds.hip).
//
// A path depends on S0, r, sigma, T, the seed and the stream alone; a policy only says where it STOPS.  So the bodies below
// take every step once -- the Model's start, reset, draw, step and index are the single sweeps', every spot is the
// generator's -- and keep, per entry e < E, what bounds_lower_body / bounds_inner_body keep for their one policy: the index
// each partner stopped at, the stop dates, the sums.  bd_mark, bd_stop and bd_value are the single sweeps' own functions,
// handed the entry's view of the arguments (cb_entry: K, invK, is_put, betas), so an irregular date decides with the float64
// rule on the entry's own fits exactly as bd_stop does.
//   lower   an entry's three sums are accumulated per thread over the same strided pair loop and reduced by the same
//           block_reduce8 into the same bounds_lower_blocks slots: they carry the bits of that entry's bounds_lower.
//   inner   a lane is finished when both partners have stopped under EVERY entry; its value under entry e is
//           bd_value(xa, da) + bd_value(xb, db), the single sweep's expression (cb_pair_value).  While no lane is refilled
//           (half_inner <= 64) every lane holds one pair value per entry and wave_sum_f64 has a fixed order: Q^ carries the
//           single call's bits.
//           With refills the lanes take the later pairs in another order than under one policy (a lane is free only once
//           its LAST entry has stopped), so Q^ differs from the single call's by the order of a float64 sum of non-negative
//           terms.  The stops do not: an entry's integer step count equals its single call's.
// E is a template argument: the per-entry state lives in registers, indexed by unrolled loops.
#pragma once
#include "omc_bounds_dev.h"
#include "omc_chain_bounds.h"

namespace omc {

// the arguments as entry e's single sweep would see them (only what bd_stop and bd_value read differs)
__device__ __forceinline__ BoundsArgs cb_entry(const BoundsArgs& c, const ChainBoundsEntry& e)
{
    BoundsArgs a = c;
    a.K = e.K;
    a.invK = e.invK;
    a.is_put = e.is_put;
    a.betas = e.betas;
    return a;
}

// bd_value(xa, da) + bd_value(xb, db) with its rounding pinned.  The compiler contracts that sum to ONE fused multiply-add and
// is free to pick the product it fuses; the single sweeps' kernels compile to fma(D[da], Z_a, D[db] Z_b) -- the first
// partner's product fused, the second's rounded -- and with several entries side by side the choice otherwise varies from
// entry to entry (seen: one entry of two, the last bit of a lower bound).  Written out, every entry gets the single form.
__device__ __forceinline__ double cb_pair_value(float xa, int da, float xb, int db, const BoundsArgs& a)
{
    const double pa = payoff_d(xa, a.K, a.is_put);
    return __builtin_fma(a.D[da], pa > 0.0 ? pa : 0.0, bd_value(xb, db, a));
}

// the entries' stored-path tables [N+1][8] -> LDS [E][N+1][4]
template <int E>
__device__ __forceinline__ void cb_load_tables(const ChainBoundsGroup& g, int N, uint4* sh)
{
#pragma unroll
    for (int e = 0; e < E; ++e)
        for (int t = threadIdx.x; t <= N; t += blockDim.x)
            sh[(size_t)e * (size_t)(N + 1) + t] = *reinterpret_cast<const uint4*>(g.e[e].tab + (size_t)t * 8);
    __syncthreads();
}

// is a partner still live under some entry?  (stop dates are >= 1, 0 while live)
template <int E>
__device__ __forceinline__ bool cb_any_live(const int (&da)[E], const int (&db)[E])
{
    int mn = da[0] < db[0] ? da[0] : db[0];
#pragma unroll
    for (int e = 1; e < E; ++e) {
        mn = da[e] < mn ? da[e] : mn;
        mn = db[e] < mn ? db[e] : mn;
    }
    return mn == 0;
}

// ------------------------------------------------------------------ lower bound
// one thread per antithetic pair of fresh paths, as bounds_lower_body; sh_bt [E][N+1] dynamic LDS, red [kNQ * kRedStride]
template <class Model, int E>
__device__ __forceinline__ void chain_bounds_lower_body(const BoundsArgs& c, const ChainBoundsGroup& g, const Model& m, int nblk,
                                                        uint4* sh_bt, double* red)
{
    cb_load_tables<E>(g, c.N, sh_bt);
    const int N = c.N;
    const int n1 = N + 1;
    double acc[E][3];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e][0] = acc[e][1] = acc[e][2] = 0.0;
    const int64_t P = c.n_lower / 2;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < P; p += (int64_t)nblk * kBlock) {
        typename Model::Spots s;
        m.reset(s, m.lower_start());
        float xa[E], xb[E];
        int da[E], db[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            xa[e] = xb[e] = 0.0f;
            da[e] = db[e] = 0;
        }
        // while some entry has a live partner; every entry stops at d = N (bd_stop), so the loop ends with the blocks
        for (int blk = 0; 4 * blk < N && cb_any_live<E>(da, db); ++blk) {
            typename Model::Normals z;
            m.draw((uint64_t)p, (uint32_t)blk, c.stream_lower, z);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int d = 4 * blk + u + 1;
                if (d > N) break;
                m.step(s, z, u);
                const float ia = m.index_a(s), ib = m.index_b(s);
#pragma unroll
                for (int e = 0; e < E; ++e) bd_mark(ia, ib, d, sh_bt[e * n1 + d], cb_entry(c, g.e[e]), xa[e], xb[e], da[e], db[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const BoundsArgs a = cb_entry(c, g.e[e]);
            const double v = 0.5 * cb_pair_value(xa[e], da[e], xb[e], db[e], a);
            acc[e][0] += v;
            acc[e][1] = __builtin_fma(v, v, acc[e][1]);  // (the single sweep's v * v is contracted into its sum likewise)
            acc[e][2] += (da[e] < N ? 1.0 : 0.0) + (db[e] < N ? 1.0 : 0.0);
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {  // the single sweep's reduction, entry by entry
        double full[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) full[q] = q < 3 ? acc[e][q] : 0.0;
        const double r = block_reduce8(full, red);
        if (threadIdx.x < 64 && (threadIdx.x & 7) == 0) g.e[e].part[(size_t)(threadIdx.x >> 3) * kPStride + blockIdx.x] = r;
        __syncthreads();  // red is reused by the next entry
    }
}

// ------------------------------------------------------------------ inner simulations
// items, waves, lanes and the refill as bounds_inner_body; sh_bt [E][N+1] dynamic LDS
template <class Model, int E>
__device__ __forceinline__ void chain_bounds_inner_body(const BoundsArgs& c, const ChainBoundsGroup& g, const Model& m, int64_t i0,
                                                        int64_t ni, uint4* sh_bt)
{
    cb_load_tables<E>(g, c.N, sh_bt);
    const int N = c.N;
    const int n1 = N + 1;
    const int lane = (int)(threadIdx.x & 63);
    const int64_t H = c.half_inner;
    const int64_t n_items = ni * N;
    const int64_t nwaves = (int64_t)gridDim.x * (kBlock / 64);
    unsigned long long steps[E], sim = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) steps[e] = 0;
    for (int64_t item = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); item < n_items; item += nwaves) {
        const int t = (int)(item / ni);
        const int64_t i = i0 + (item - (int64_t)t * ni);
        const typename Model::Start s0 = m.inner_start(t, i);
        const uint64_t gbase = ((uint64_t)i * (uint64_t)(N + 1) + (uint64_t)t) * (uint64_t)H;
        int64_t j = lane, next = 64;  // this lane's pair; the item's first unstarted pair
        bool act = j < H;
        typename Model::Spots s;
        m.reset(s, s0);
        float xa[E], xb[E];
        int da[E], db[E];  // stop dates of the pair's partners under each entry (0 while live)
        double acc[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            xa[e] = xb[e] = 0.0f;
            da[e] = db[e] = 0;
            acc[e] = 0.0;
        }
        int k = 0;  // steps taken by the pair
        while (__builtin_amdgcn_ballot_w64(act)) {
            if (act) {
                typename Model::Normals z;
                m.draw(gbase + (uint64_t)j, (uint32_t)(k >> 2), c.stream_inner, z);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    // a step is taken while some entry has a live partner.  Every entry stops at d >= N (bd_stop returns
                    // true there), so no pair steps past date N: at most N - t steps, the single sweep's worst case
                    if (cb_any_live<E>(da, db)) {
                        ++k;
                        const int d = t + k;
                        m.step(s, z, u);
                        const float ia = m.index_a(s), ib = m.index_b(s);
#pragma unroll
                        for (int e = 0; e < E; ++e)
                            bd_mark(ia, ib, d, sh_bt[e * n1 + d], cb_entry(c, g.e[e]), xa[e], xb[e], da[e], db[e]);
                    }
                }
            }
            const bool done = act && !cb_any_live<E>(da, db);
            const uint64_t fin = __builtin_amdgcn_ballot_w64(done);
            if (done) {
                int ma = 0, mb = 0;  // the partners' last stops: the steps that were simulated
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const BoundsArgs a = cb_entry(c, g.e[e]);
                    acc[e] += cb_pair_value(xa[e], da[e], xb[e], db[e], a);
                    steps[e] += (unsigned long long)(da[e] - t) + (unsigned long long)(db[e] - t);
                    ma = da[e] > ma ? da[e] : ma;
                    mb = db[e] > mb ? db[e] : mb;
                    xa[e] = xb[e] = 0.0f;
                    da[e] = db[e] = 0;
                }
                sim += (unsigned long long)(ma - t) + (unsigned long long)(mb - t);
                // the finished lanes take the next pairs in lane order (mbcnt: finished lanes below this one)
                j = next + (int64_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(fin >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fin, 0));
                act = j < H;
                m.reset(s, s0);
                k = 0;
            }
            next += __popcll(fin);
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const double q = wave_sum_f64(acc[e]);
            if (lane == 0) g.e[e].q[(size_t)i * N + t] = q / (double)(2 * H);
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) steps[e] += __shfl_xor(steps[e], off, 64);
        if (lane == 0 && steps[e]) atomicAdd(g.e[e].steps, steps[e]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sim += __shfl_xor(sim, off, 64);
    if (lane == 0 && sim) atomicAdd(g.steps_sim, sim);
}

}  // namespace omc
