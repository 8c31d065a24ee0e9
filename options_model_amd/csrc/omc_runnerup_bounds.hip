// omc_runnerup_bounds.hip -- Andersen-Broadie price bounds of best-of / worst-of options on D correlated GBM assets with a
// policy that sees the index X AND the runner-up Y, the second order statistic of the weighted spots (DESIGN.md section 18;
// the definitions are include/omc.h's).
//
//   fit     classic Longstaff-Schwartz on the generator's kept asset matrices, one launch per date t = N-1 .. 1 that
//           applies the rule of date t+1 to the path state (x_ex, tex) and leaves the 27 sums of date t's regression per
//           workgroup, and a one-workgroup launch that adds them in a fixed order and solves the centred 5 x 5 system.
//   lower   omc_basket_bounds.hip's lower sweep with the two-regressor stop.
//   inner   the hot path, omc_basket_bounds.hip's inner simulations with the two-regressor stop.
//   walk    omc_bounds.hip's outer walk with the two-regressor stop on (Xo, Yo), Yo from the outer asset matrices.
// The lower sweep and the inner simulations RESTATE bounds_lower_body / bounds_inner_body (omc_bounds_dev.h) -- the loops,
// the stop bookkeeping, the ballot + mbcnt refill, the xor-shuffle sum and the step count are theirs, line for line; a change
// to either must be made here too.  They are restated and not shared because those bodies hand the policy ONE float32 per
// partner and decide from a uint4 table row in LDS; here a date's row is 64 bytes of float64 coefficients, the policy takes
// a pair of values, and the float64 polynomial sits behind a wave-uniform branch.  The walk restates bd_sample likewise.
// Every spot is the basket generator's (omc_basket_dev.h), X has the bits of basket_law_index, the sums are float64 in a
// fixed order: identical calls return identical bits.  D is a template parameter and the law comes by value, so every loop
// over assets unrolls and nothing is indexed at run time (no scratch).
#include "omc_runnerup_bounds.h"
#include "omc_basket_dev.h"
#include "omc_bounds_dev.h"

namespace omc {

struct XY {
    float x, y;  // the index and the runner-up
};

// (X, Y) of one path in one pass over v_k = w_k s_k: a compare, two selects and one max (min) per asset.  Y counts with
// multiplicity (a tie v == X leaves X and makes Y = X); X is the fmaxf / fminf chain of basket_index bit for bit: the v_k are
// positive and finite.
template <bool BEST, int D>
__device__ __forceinline__ XY ru_xy_kind(const BasketLaw& c, const float (&s)[D])
{
    float x = c.w[0] * s[0];
    float y = BEST ? -__builtin_huge_valf() : __builtin_huge_valf();
#pragma unroll
    for (int k = 1; k < D; ++k) {
        const float v = c.w[k] * s[k];
        const bool lead = BEST ? v > x : v < x;
        const float rest = BEST ? fmaxf(y, v) : fminf(y, v);
        y = lead ? x : rest;
        x = lead ? v : x;
    }
    return {x, y};
}

// ... of the law's own kind (wave-uniform: a scalar branch)
template <int D>
__device__ __forceinline__ XY ru_xy(const BasketLaw& c, const float (&s)[D])
{
    if (c.kind == OMC_BASKET_BEST_OF) return ru_xy_kind<true, D>(c, s);
    return ru_xy_kind<false, D>(c, s);
}

// (X, Y) of column j, row t of kept asset matrices A [D][rows][ld] (stride: one asset's matrix)
template <int D>
__device__ __forceinline__ XY ru_xy_stored(const BasketLaw& c, const float* __restrict__ A, size_t stride, size_t at)
{
    float s[D];
#pragma unroll
    for (int k = 0; k < D; ++k) s[k] = A[(size_t)k * stride + at];
    return ru_xy<D>(c, s);
}

struct RuRule {
    double K, invK;
    float thr;  // phi(X) > 0 as one float32 compare (itm_threshold)
    int is_put, N;
};
__device__ __forceinline__ RuRule ru_rule(double K, double invK, int is_put, int N)
{
    return {K, invK, itm_threshold(K, is_put), is_put, N};
}
__device__ __forceinline__ bool ru_itm(float x, const RuRule& r) { return r.is_put ? x < r.thr : x > r.thr; }

// the float64 rule of a date t in 1 .. N-1 with the date's row (c0 .. c5, n, 0)
__device__ __forceinline__ bool ru_exercises(XY p, const double* row, const RuRule& r)
{
    const double imm = payoff_d(p.x, r.K, r.is_put);
    const double u = fma((double)p.x, r.invK, -1.0), w = fma((double)p.y, r.invK, -1.0);
    const double cont = fma(w, fma(w, row[4], fma(u, row[5], row[3])), fma(u, fma(u, row[2], row[1]), row[0]));
    return (row[6] > 0.5) & (imm > 0.0) & (imm > cont);
}

// the policy rows [N+1][8] -> LDS
__device__ __forceinline__ void ru_load_policy(const double* __restrict__ pol, int N, double* sh)
{
    for (int i = threadIdx.x; i < (N + 1) * kRunnerupCols; i += blockDim.x) sh[i] = pol[i];
    __syncthreads();
}

// bd_mark with the two-regressor stop: one step of both partners' stop bookkeeping at date d.  The float64 polynomial runs
// only when a live partner of some lane of the wave is in the money at a date before N (ballot: a scalar branch)
__device__ __forceinline__ void ru_mark(XY pa, XY pb, int d, const double* sh_pol, const RuRule& r, float& xa, float& xb,
                                        int& da, int& db)
{
    bool ea = da == 0, eb = db == 0;
    if (d < r.N) {
        ea = ea && ru_itm(pa.x, r);
        eb = eb && ru_itm(pb.x, r);
        if (__builtin_amdgcn_ballot_w64(ea || eb)) {
            const double* row = sh_pol + (size_t)d * kRunnerupCols;
            ea = ea && ru_exercises(pa, row, r);
            eb = eb && ru_exercises(pb, row, r);
        }
    }
    xa = ea ? pa.x : xa;
    da = ea ? d : da;
    xb = eb ? pb.x : xb;
    db = eb ? d : db;
}

// ------------------------------------------------------------------ lower bound (bounds_lower_body, restated)
template <int D>
__global__ __launch_bounds__(kBlock) void runnerup_lower_kernel(RunnerupArgs g, int nblk)
{
    extern __shared__ double sh_pol[];
    __shared__ double red[kNQ * kRedStride];
    const BoundsArgs& a = g.g.v;
    const BasketLaw& c = g.g.law;
    ru_load_policy(g.pol, a.N, sh_pol);
    const RuRule rule = ru_rule(a.K, a.invK, a.is_put, a.N);
    const int N = a.N;
    double acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0;
    const int64_t P = a.n_lower / 2;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < P; p += (int64_t)nblk * kBlock) {
        float sa[D], sb[D];
#pragma unroll
        for (int k = 0; k < D; ++k) sa[k] = sb[k] = c.s0[k];
        float xa = 0.0f, xb = 0.0f;  // the index each partner stopped at (written by the stop that sets da / db)
        int da = 0, db = 0;          // stop dates, 0 while live
        for (int blk = 0; 4 * blk < N && (da == 0 || db == 0); ++blk) {
            float y[D][4];
            basket_normals<D>(c, (uint64_t)p, (uint32_t)blk, a.stream_lower, a.k0, a.k1, y);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int d = 4 * blk + u + 1;
                if (d > N) break;
                basket_step<D>(c, sa, sb, y, u);
                ru_mark(ru_xy<D>(c, sa), ru_xy<D>(c, sb), d, sh_pol, rule, xa, xb, da, db);
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

// ------------------------------------------------------------------ inner simulations (bounds_inner_body, restated)
// items q = t * ni + (i - i0); a wave owns one item at a time, a lane one antithetic inner pair: 2 D asset spots and 4 D
// correlated normals per lane.  The item's D start spots are the outer ASSET spots A_k[t][i], held as scalars
template <int D>
__global__ __launch_bounds__(kBlock) void runnerup_inner_kernel(RunnerupArgs g, int64_t i0, int64_t ni)
{
    extern __shared__ double sh_pol[];
    const BoundsArgs& a = g.g.v;
    const BasketLaw& c = g.g.law;
    ru_load_policy(g.pol, a.N, sh_pol);
    const RuRule rule = ru_rule(a.K, a.invK, a.is_put, a.N);
    const int N = a.N;
    const int lane = (int)(threadIdx.x & 63);
    const int64_t H = a.half_inner;
    const int64_t n_items = ni * N;
    const int64_t nwaves = (int64_t)gridDim.x * (kBlock / 64);
    const size_t astride = (size_t)(N + 1) * (size_t)a.n_outer;  // one asset's outer matrix
    unsigned long long steps = 0;
    for (int64_t item = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); item < n_items; item += nwaves) {
        const int t = (int)(item / ni);
        const int64_t i = i0 + (item - (int64_t)t * ni);
        float s0[D];  // the item's start spots: one address per wave, held as scalars
#pragma unroll
        for (int k = 0; k < D; ++k)
            s0[k] = __int_as_float(
                __builtin_amdgcn_readfirstlane(__float_as_int(g.g.Ao[(size_t)k * astride + (size_t)t * a.n_outer + i])));
        const uint64_t gbase = ((uint64_t)i * (uint64_t)(N + 1) + (uint64_t)t) * (uint64_t)H;
        int64_t j = lane, next = 64;  // this lane's pair; the item's first unstarted pair
        bool act = j < H;
        float sa[D], sb[D], xa = 0.0f, xb = 0.0f;
#pragma unroll
        for (int k = 0; k < D; ++k) sa[k] = sb[k] = s0[k];
        int k = 0, da = 0, db = 0;  // steps taken by the pair; stop dates of its partners (0 while live)
        double acc = 0.0;
        while (__builtin_amdgcn_ballot_w64(act)) {
            if (act) {
                float y[D][4];
                basket_normals<D>(c, gbase + (uint64_t)j, (uint32_t)(k >> 2), a.stream_inner, a.k0, a.k1, y);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (da == 0 || db == 0) {
                        ++k;
                        const int d = t + k;
                        basket_step<D>(c, sa, sb, y, u);
                        ru_mark(ru_xy<D>(c, sa), ru_xy<D>(c, sb), d, sh_pol, rule, xa, xb, da, db);
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
#pragma unroll
                for (int q = 0; q < D; ++q) sa[q] = sb[q] = s0[q];
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

// ------------------------------------------------------------------ outer walk (bd_sample / bounds_walk_kernel, restated)
template <int D>
__device__ __forceinline__ double ru_sample(const RunnerupArgs& g, const RuRule& rule, int64_t i)
{
#pragma clang fp contract(off)
    const BoundsArgs& a = g.g.v;
    const int N = a.N;
    const size_t astride = (size_t)(N + 1) * (size_t)a.n_outer;
    const double* q = a.q + (size_t)i * N;
    double M = 0.0, qprev = q[0], best = -__builtin_huge_val();
    for (int t = 1; t <= N; ++t) {
        const XY p = ru_xy_stored<D>(g.g.law, g.g.Ao, astride, (size_t)t * a.n_outer + i);
        double pay = payoff_d(p.x, a.K, a.is_put);
        pay = pay > 0.0 ? pay : 0.0;
        const double Dt = a.D[t], Z = Dt * pay;  // bd_value
        const double qt = t < N ? q[t] : 0.0;
        const bool stop = t >= N || (ru_itm(p.x, rule) && ru_exercises(p, g.pol + (size_t)t * kRunnerupCols, rule));
        const double L = stop ? Z : qt;
        M = M + L - qprev;
        // Z - M as bounds_walk_kernel computes it: there the compiler contracts the product of Z into the subtraction.  Spelled
        // out (and nothing else contracted: the pragma above), so that equal decisions give the index walk's bits
        const double x = fma(Dt, pay, -M);
        best = x > best ? x : best;
        qprev = qt;
    }
    return best;
}

template <int D>
__global__ __launch_bounds__(kBlock) void runnerup_walk_kernel(RunnerupArgs g, int nblk)
{
    __shared__ double red[kNQ * kRedStride];
    const BoundsArgs& a = g.g.v;
    const RuRule rule = ru_rule(a.K, a.invK, a.is_put, a.N);
    double acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.0;
    const int64_t P = a.n_outer / 2;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < P; p += (int64_t)nblk * kBlock) {
        const double xa = ru_sample<D>(g, rule, p), xb = ru_sample<D>(g, rule, p + P);
        a.samples[p] = xa;
        a.samples[p + P] = xb;
        const double m = 0.5 * (xa + xb);
        acc[0] += m;
        acc[1] += m * m;
    }
    const double s = block_reduce8(acc, red);
    if (threadIdx.x < 64 && (threadIdx.x & 7) == 0) a.part[(size_t)(threadIdx.x >> 3) * kPStride + blockIdx.x] = s;
}

// ------------------------------------------------------------------ the fit
// Date t of classic Longstaff-Schwartz (semantics 1 of lsm_step_body) on the kept asset matrices.  Every path first applies
// the rule of date t+1, solved by the launch before this one, to its state (x_ex, tex) -- at t = N-1 the state starts at
// (X_N, N) --; the paths with phi(X_t) > 0 then add y = D[tex - t] max(phi(x_ex), 0) and f = (u, u^2, w, w^2, uw) to the 27
// sums: per thread in column order, per workgroup by block_reduce8 in four groups of eight.
template <int D>
__global__ __launch_bounds__(kBlock) void runnerup_fit_sums_kernel(RunnerupFit f, int t, int nblk)
{
    __shared__ double red[kNQ * kRedStride];
    const RuRule rule = ru_rule(f.K, f.invK, f.is_put, f.N);
    const size_t astride = (size_t)(f.N + 1) * (size_t)f.ld;
    const bool init = t == f.N - 1;
    double row[kRunnerupCols];
#pragma unroll
    for (int q = 0; q < kRunnerupCols; ++q) row[q] = init ? 0.0 : f.pol[(size_t)(t + 1) * kRunnerupCols + q];
    double acc[kRunnerupSlots];
#pragma unroll
    for (int q = 0; q < kRunnerupSlots; ++q) acc[q] = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < f.M; j += (int64_t)nblk * kBlock) {
        const XY next = ru_xy_stored<D>(f.law, f.A, astride, (size_t)(t + 1) * f.ld + j);
        float xe = next.x;
        int32_t te = t + 1;
        bool changed = true;
        if (!init) {
            changed = ru_itm(next.x, rule) && ru_exercises(next, row, rule);
            xe = changed ? next.x : f.x_ex[j];
            te = changed ? t + 1 : f.tex[j];
        }
        if (changed) {
            f.x_ex[j] = xe;
            f.tex[j] = te;
        }
        const XY p = ru_xy_stored<D>(f.law, f.A, astride, (size_t)t * f.ld + j);
        if (ru_itm(p.x, rule)) {
            double pay = payoff_d(xe, f.K, f.is_put);
            pay = pay > 0.0 ? pay : 0.0;
            const double y = f.D[te - t] * pay;
            const double u = fma((double)p.x, f.invK, -1.0), w = fma((double)p.y, f.invK, -1.0);
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

// The sums m [27] of a date -> its policy row (c0 .. c5, n, 0): the centred system C = sum f f' - sum f sum f' / n,
// c = sum f y - sum f sum y / n by LDL' without pivoting in the order of f, with solve_poly2's truncation rule carried
// over: feature j (from 0) and everything after it get coefficient 0 when n < j + 1.5 or the pivot is not above
// 1e-12 |C_jj| + 1e-300.  One thread; its small matrices live in LDS (w), so nothing is indexed in registers.
struct RuSolveLds {
    double C[5][5], L[5][5], c[5], fbar[5], dd[5], z[5], x[5];
};
__device__ void ru_solve(const double* m, RuSolveLds& w, double* out)
{
    const double n = m[0];
    for (int q = 0; q < kRunnerupCols; ++q) out[q] = 0.0;
    if (n < 0.5) return;
    out[6] = n;
    const double ybar = m[21] / n;
    int q = 6;
    for (int a = 0; a < 5; ++a) {
        w.fbar[a] = m[1 + a] / n;
        w.c[a] = m[22 + a] - m[1 + a] * ybar;
        w.x[a] = 0.0;
    }
    for (int a = 0; a < 5; ++a)
        for (int b = a; b < 5; ++b) w.C[a][b] = w.C[b][a] = m[q++] - m[1 + a] * w.fbar[b];
    int kept = 0;
    for (int j = 0; j < 5; ++j) {
        for (int i = 0; i < j; ++i) {
            double s = w.C[j][i];
            for (int l = 0; l < i; ++l) s -= w.L[j][l] * w.L[i][l] * w.dd[l];
            w.L[j][i] = s / w.dd[i];
        }
        double piv = w.C[j][j];
        for (int l = 0; l < j; ++l) piv -= w.L[j][l] * w.L[j][l] * w.dd[l];
        if (n < (double)j + 1.5 || !(piv > 1e-12 * fabs(w.C[j][j]) + 1e-300)) break;
        w.dd[j] = piv;
        kept = j + 1;
    }
    for (int j = 0; j < kept; ++j) {
        double s = w.c[j];
        for (int l = 0; l < j; ++l) s -= w.L[j][l] * w.z[l];
        w.z[j] = s;
    }
    for (int j = kept - 1; j >= 0; --j) {
        double s = w.z[j] / w.dd[j];
        for (int l = j + 1; l < kept; ++l) s -= w.L[l][j] * w.x[l];
        w.x[j] = s;
    }
    double c0 = ybar;
    for (int j = 0; j < kept; ++j) c0 -= w.x[j] * w.fbar[j];
    out[0] = c0;
    for (int j = 0; j < 5; ++j) out[1 + j] = w.x[j];
}

// one workgroup: thread (q, sub) adds every eighth partial of sum q, the eight of a sum meet in sum_group8, thread 0 solves
__global__ __launch_bounds__(kBlock) void runnerup_fit_solve_kernel(const double* __restrict__ part, int nblk, double* row)
{
    __shared__ double m[kRunnerupSlots];
    __shared__ RuSolveLds w;
    const int q = threadIdx.x >> 3, sub = threadIdx.x & 7;
    double s = 0.0;
    for (int i = sub; i < nblk; i += 8) s += part[(size_t)q * kRunnerupFitBlocks + i];
    s = sum_group8(s);
    if (sub == 0) m[q] = s;
    __syncthreads();
    if (threadIdx.x == 0) ru_solve(m, w, row);
}

// ------------------------------------------------------------------ launchers
static bool ru_assets_ok(int d) { return d >= 2 && d <= kBasketMax; }

hipError_t runnerup_fit(hipStream_t st, const RunnerupFit& f)
{
    static_assert(kRunnerupSlots * 8 == kBlock, "one thread per (sum, eighth) in the solve launch");
    if (!ru_assets_ok(f.d)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(f.pol, 0, sizeof(double) * kRunnerupCols * (size_t)(f.N + 1), st);
    if (e != hipSuccess) return e;
    int64_t nb = (f.M + kBlock - 1) / kBlock;
    const int nblk = (int)(nb < kRunnerupFitBlocks ? nb : kRunnerupFitBlocks);
    for (int t = f.N - 1; t >= 1; --t) {
        for_runnerup_assets(f.d, [&](auto d) {
            hipLaunchKernelGGL((runnerup_fit_sums_kernel<d()>), dim3(nblk), dim3(kBlock), 0, st, f, t, nblk);
        });
        hipLaunchKernelGGL(runnerup_fit_solve_kernel, dim3(1), dim3(kBlock), 0, st, f.part, nblk,
                           f.pol + (size_t)t * kRunnerupCols);
    }
    return hipGetLastError();
}

hipError_t runnerup_fit_solve(hipStream_t st, const double* part, int nblk, double* row)
{
    if (nblk < 1 || nblk > kRunnerupFitBlocks) return hipErrorInvalidValue;
    hipLaunchKernelGGL(runnerup_fit_solve_kernel, dim3(1), dim3(kBlock), 0, st, part, nblk, row);
    return hipGetLastError();
}

static size_t ru_policy_lds(const RunnerupArgs& a) { return sizeof(double) * kRunnerupCols * (size_t)(a.g.v.N + 1); }

hipError_t runnerup_lower(hipStream_t st, const RunnerupArgs& a, double* result)
{
    if (!ru_assets_ok(a.g.d) || a.g.v.N > kRunnerupMaxSteps) return hipErrorInvalidValue;
    const int nblk = (int)bounds_lower_blocks(a.g.v);  // the vanilla sweep's grid
    for_runnerup_assets(a.g.d, [&](auto d) {
        hipLaunchKernelGGL((runnerup_lower_kernel<d()>), dim3(nblk), dim3(kBlock), ru_policy_lds(a), st, a, nblk);
    });
    return lsm_finalize(st, a.g.v.part, nullptr, result, nblk, 0);
}

hipError_t runnerup_inner(hipStream_t st, const RunnerupArgs& a, int64_t i0, int64_t ni)
{
    if (!ru_assets_ok(a.g.d) || a.g.v.N > kRunnerupMaxSteps) return hipErrorInvalidValue;
    const unsigned g = bounds_inner_grid(ni * a.g.v.N);
    for_runnerup_assets(a.g.d, [&](auto d) {
        hipLaunchKernelGGL((runnerup_inner_kernel<d()>), dim3(g), dim3(kBlock), ru_policy_lds(a), st, a, i0, ni);
    });
    return hipGetLastError();
}

hipError_t runnerup_walk(hipStream_t st, const RunnerupArgs& a, double* result)
{
    if (!ru_assets_ok(a.g.d)) return hipErrorInvalidValue;
    const int nblk = (int)bounds_walk_blocks(a.g.v);
    for_runnerup_assets(a.g.d, [&](auto d) {
        hipLaunchKernelGGL((runnerup_walk_kernel<d()>), dim3(nblk), dim3(kBlock), 0, st, a, nblk);
    });
    return lsm_finalize(st, a.g.v.part, nullptr, result, nblk, 0);
}

}  // namespace omc
