// omc_chain.hip -- the option-chain kernels for gfx950 (omc_price_american_chain): many strikes and
// sides of one expiry priced from ONE folded path matrix.
//
// The paths depend on neither the strike nor the side, and on folded storage neither does C_t = S0^2 exp(2 drift t): only
// cK[t] = C_t / K does.  The two sweeps of the single pricing (lsm_pass1_fold_body, lsm_pass2_fold_body) are bound by vector
// issue, and a good part of what they issue per spot -- the load and its address arithmetic, the float -> double
// conversion, the v_rcp_f64 + Newton reciprocal behind the partner's moneyness, the look-ahead walk -- does not depend on
// the strike.  The chain sweeps spend that once per spot for all entries of a launch:
//   lsm_pass1_fold_chain_kernel   the geometry of lsm_pass1_fold_body (wave x TPW tiles x a chunk of steps, rows requested two
//                                 steps ahead); per entry its own 8 accumulators, wave_reduce8 and part1 slab
//   lsm_pass2_fold_chain_kernel   a thread walks its stored columns backward ONCE and decides at every row for every entry
//                                 from that entry's exercise tables in LDS; per entry its own (sxa, sxb, texa, texb),
//                                 its own add_cash_flow sequence and block_reduce8
// Per entry every sum is formed over the same operands in the same order as by the single kernels -- same tiles, blocks
// and slots (lsm_fold_geometry), same expressions (omc_lsm_dev.h) -- so an entry's partials, hence its moments, fits, tables
// and result, carry the bits of its own omc_price_american call.
#include "omc_chain.h"
#include "omc_lsm_dev.h"

#include <cstdint>

namespace omc {

// ------------------------------------------------------------------ fold tables, one per entry
__global__ __launch_bounds__(64) void chain_fold_tables_kernel(double* __restrict__ cK, size_t stride,
                                                                const double* __restrict__ c0, int n, int N, double g)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= n) return;
    fold_table_fill(cK + (size_t)j * stride, N, c0[j], g);
}

hipError_t chain_fold_tables(hipStream_t st, double* cK, size_t stride, const double* c0, int n, int N, double g)
{
    hipLaunchKernelGGL(chain_fold_tables_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, cK, stride, c0, n, N, g);
    return hipGetLastError();
}

// ------------------------------------------------------------------ Bermudan entries: the tables on the scheduled rows
// One workgroup per entry, one thread per row j = 0 .. Nv of its view (omc_chain.h).  Indices that fall outside a table
// (d1 at j = Nv and d2 at j = Nv when k > 1, the view's row 0 above the matrix) are slots no sweep reads: they are
// clamped into the table, not skipped, so every slot holds a finite number.
__global__ __launch_bounds__(64) void chain_schedule_tables_kernel(double* __restrict__ out, size_t stride,
                                                                    const double* __restrict__ D,
                                                                    const double* __restrict__ cK, size_t cstride,
                                                                    ChainSchedules s, int N)
{
    const int i = (int)blockIdx.x, k = s.every[i];
    if (k < 2 || k > N) return;
    const int Nv = chain_view_steps(N, k);
    double* d1 = out + 3 * stride * (size_t)i;
    double* d2 = d1 + stride;
    double* cv = d2 + stride;
    const double* ci = cK ? cK + cstride * (size_t)i : nullptr;
    for (int j = (int)threadIdx.x; j <= Nv; j += 64) {
        const int row = N - k * (Nv - j);  // >= 1 for j >= 1, == N for j == Nv
        d1[j] = D[min(k * j, N)];
        d2[j] = D[min(row + k - 1, N)];
        if (ci) cv[j] = ci[max(row, 0)];
    }
}

hipError_t chain_schedule_tables(hipStream_t st, double* out, size_t stride, const double* D, const double* cK,
                                 size_t cstride, const ChainSchedules& s, int n, int N)
{
    if (n < 1 || n > kChainMax || stride < (size_t)N + 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(chain_schedule_tables_kernel, dim3((unsigned)n), dim3(64), 0, st, out, stride, D, cK, cstride, s, N);
    return hipGetLastError();
}

// one workgroup per member of the group, one thread per quantity: the rows of a column are moved one after the other
__global__ __launch_bounds__(64) void chain_gather_moments_kernel(ChainGatherArgs a)
{
    const int m = (int)blockIdx.x, k = a.every[m], q = (int)threadIdx.x;
    if (k < 2 || k > a.N || q >= 8) return;
    const int Nv = chain_view_steps(a.N, k);
    double* g = a.gmom[m];
    for (int j = 1; j < Nv; ++j) g[(size_t)j * 8 + q] = g[(size_t)(a.N - k * (Nv - j)) * 8 + q];
}

hipError_t chain_gather_moments(hipStream_t st, const ChainGatherArgs& a, int K)
{
    if (K < 1 || K > kChainGroupMax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(chain_gather_moments_kernel, dim3((unsigned)K), dim3(64), 0, st, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------ pass 1, KE entries of one side per launch
// lsm_pass1_fold_body with an entry loop inside every step.  Per spot, once: the conversion and the reciprocal (fold_rcp);
// per entry: both moneynesses (fold_u_rcp keeps the partner's the fma(cK, rcp, -1) of fold_u), the two in-the-money tests,
// the row sums.  Terminal payoffs are RECOMPUTED per entry and step from the terminal row (its float64 spots and their
// reciprocals stay in registers: 4 doubles per stored column against 2 per column AND entry for the payoffs themselves).
// The chunk's discount factors and every entry's cK row are shared by the workgroup's four waves (one barrier in the
// prologue; none afterwards).
template <int VEC, int TPW, int PUT>
__global__ __launch_bounds__(kBlock) void lsm_pass1_fold_chain_kernel(ChainSweepArgs a, int64_t ntiles, int tchunk)
{
    __shared__ double wl[kBlock / 64][kWaveRedDoubles];
    __shared__ double shD[kFoldMaxChunk];
    __shared__ double shC[kChainWidthMax][kFoldMaxChunk];
    __shared__ double shE[kChainWidthMax][4];  // K, 1 / K, cK[N], the float32 in-the-money threshold
    constexpr bool IS_PUT = PUT != 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = a.N, KE = a.KE;
    const int t0 = 1 + ((int)gridDim.y - 1 - (int)blockIdx.y) * tchunk;
    const int t1 = min(t0 + tchunk, N);
    if (t0 >= t1) return;  // (the whole workgroup)
    for (int i = threadIdx.x; i < t1 - t0; i += kBlock) shD[i] = a.D[N - (t0 + i)];
    for (int e = 0; e < KE; ++e) {
        const double* cKe = a.cK[e];
        for (int i = threadIdx.x; i < t1 - t0; i += kBlock) shC[e][i] = cKe[t0 + i];
        if (threadIdx.x == 0) {
            shE[e][0] = a.K[e];
            shE[e][1] = a.invK[e];
            shE[e][2] = cKe[N];
            shE[e][3] = (double)itm_threshold(a.K[e], PUT);
        }
    }
    __syncthreads();
    const int64_t tg = (int64_t)xcd_block((int)blockIdx.x, (int)gridDim.x) * (kBlock / 64) + wave;
    if (tg >= ntiles) return;  // whole wave leaves; no workgroup barrier below
    const int64_t base = tg * (64 * VEC * TPW) + (int64_t)lane * VEC;
    const float* colp[TPW];
    bool valid[TPW];
    double snd[TPW][VEC], rn[TPW][VEC];  // terminal spots and their reciprocals
    {
        float sn[TPW][VEC];
#pragma unroll
        for (int k = 0; k < TPW; ++k) {
            const int64_t j = base + (int64_t)k * 64 * VEC;
            valid[k] = j < a.P;
            colp[k] = a.S + (valid[k] ? j : 0);
            loadf<VEC>(colp[k] + (int64_t)N * a.ld, sn[k]);
        }
#pragma unroll
        for (int k = 0; k < TPW; ++k) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                snd[k][v] = (double)sn[k][v];
                rn[k][v] = fold_rcp(sn[k][v]);
            }
        }
    }
    auto load_rows = [&](float (&buf)[TPW][VEC], int t) {
#pragma unroll
        for (int k = 0; k < TPW; ++k) loadf_stream<VEC>(colp[k] + (int64_t)t * a.ld, buf[k]);
    };
    float bufA[TPW][VEC], bufB[TPW][VEC], bufC[TPW][VEC];
    const int tl = t1 - 1;
    load_rows(bufA, t0);
    load_rows(bufB, min(t0 + 1, tl));
    __builtin_amdgcn_sched_barrier(0);
    unsigned long long vmask[TPW];  // lanes whose columns of tile k exist
#pragma unroll
    for (int k = 0; k < TPW; ++k) vmask[k] = __builtin_amdgcn_ballot_w64(valid[k]);
    auto process = [&](const float (&buf)[TPW][VEC], int t) {
        double xs[TPW][VEC], rc[TPW][VEC];
#pragma unroll
        for (int k = 0; k < TPW; ++k) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                xs[k][v] = (double)buf[k][v];
                rc[k][v] = fold_rcp(buf[k][v]);
            }
        }
        const double d = shD[t - t0];
        for (int e = 0; e < KE; ++e) {
            const double K = shE[e][0], invK = shE[e][1], cKN = shE[e][2];
            const float thr = (float)shE[e][3];
            const double ck = shC[e][t - t0];
            double acc[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] = 0.0;
            int cnt = 0;
            // (the row sums of lsm_pass1_fold_body, expression for expression)
            auto add_row = [&](double u, double y, double m) {  // u, y already zero where m is
                const double u2 = u * u;
                acc[1] += u;
                acc[2] += u2;
                acc[3] = fma(u2, u, acc[3]);
                acc[4] = fma(u2, u2, acc[4]);
                acc[5] = fma(y, m, acc[5]);
                acc[6] = fma(u, y, acc[6]);
                acc[7] = fma(u2, y, acc[7]);
            };
#pragma unroll
            for (int k = 0; k < TPW; ++k) {
                const float thrk = valid[k] ? thr : (IS_PUT ? -__builtin_inff() : __builtin_inff());
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const float sf = buf[k][v];
                    const double pa = IS_PUT ? K - snd[k][v] : snd[k][v] - K;
                    const double pb = fold_pay(fold_u_rcp(cKN, rn[k][v]), K, PUT);
                    const double pNA = (valid[k] && pa > 0.0) ? pa : 0.0;
                    const double pNB = (valid[k] && pb > 0.0) ? pb : 0.0;
                    const double ua = fma(xs[k][v], invK, -1.0);
                    const double ub = fold_u_rcp(ck, rc[k][v]);
                    const bool ia = IS_PUT ? sf < thrk : sf > thrk;
                    const bool ibc = IS_PUT ? ub < 0.0 : ub > 0.0;
                    const unsigned long long ma = __builtin_amdgcn_ballot_w64(ia);
                    const unsigned long long mb = __builtin_amdgcn_ballot_w64(ibc) & vmask[k];
                    const bool ib = valid[k] && ibc;
                    cnt += __builtin_popcountll(ma | mb);  // rows of this spot: any + both
                    const double mp = (ia || ib) ? 1.0 : 0.0;
                    add_row((ia ? ua : ub) * mp, ia ? pNA : pNB, mp);
                    const unsigned long long bb = ma & mb;
                    if (bb != 0) {
                        asm volatile("; a lane with both partners in the money" ::);  // (keeps the branch: no if-conversion)
                        cnt += __builtin_popcountll(bb);
                        const bool both = ia && ib;
                        const double ms = both ? 1.0 : 0.0;
                        add_row(ub * ms, pNB, ms);
                    }
                }
            }
            acc[0] = lane == 0 ? (double)cnt : 0.0;
            acc[5] *= d;
            acc[6] *= d;
            acc[7] *= d;
            const double s = wave_reduce8(acc, wl[wave]);
            if ((lane & 7) == 0) a.part1[e][((size_t)t * ntiles + tg) * 8 + (lane >> 3)] = s;
        }
    };
    for (int t = t0; t < t1; t += 3) {
        load_rows(bufC, min(t + 2, tl));
        __builtin_amdgcn_sched_barrier(0);
        process(bufA, t);
        if (t + 1 < t1) {
            load_rows(bufA, min(t + 3, tl));
            __builtin_amdgcn_sched_barrier(0);
            process(bufB, t + 1);
        }
        if (t + 2 < t1) {
            load_rows(bufB, min(t + 4, tl));
            __builtin_amdgcn_sched_barrier(0);
            process(bufC, t + 2);
        }
    }
}

// ------------------------------------------------------------------ pass 2, KE entries of one side per launch
// lsm_pass2_fold_body<VEC, PUT, TAB = true> with KE sets of exercise state per thread: the tables of all entries sit in LDS
// as [t][entry][8] words (one step's words of all entries next to each other), a row is loaded once and tested against
// every entry's two intervals, the walk ends when every path of every entry has exercised.  A step some entry's table
// marks irregular is decided for THAT entry by the float64 rule (decide_f64 of the single kernel), as there.
template <int VEC, int PUT, int KE>
__global__ __launch_bounds__(kBlock) void lsm_pass2_fold_chain_kernel(ChainSweepArgs a, int nblk, int pstride)
{
    if ((int)blockIdx.x >= nblk) return;
    __shared__ double red[kNQ * kRedStride];
    extern __shared__ double sh_b[];
    uint32_t* sh_t = reinterpret_cast<uint32_t*>(sh_b);  // [N+1][KE][8]
    const int tid = threadIdx.x;
    const int N = a.N;
    int irr = 0;
#pragma unroll
    for (int e = 0; e < KE; ++e) {  // crit_load_tables per entry
        const uint32_t* tab = a.crit[e];
        for (int t = tid; t <= N; t += kBlock) {
            const uint4 x = *reinterpret_cast<const uint4*>(tab + (size_t)t * 8);
            const uint4 y = *reinterpret_cast<const uint4*>(tab + (size_t)t * 8 + 4);
            const bool bad = x.x == kCritIrregular || y.x == kCritIrregular;
            irr |= bad;
            uint32_t* o = sh_t + ((size_t)t * KE + e) * 8;
            *reinterpret_cast<uint4*>(o) = make_uint4(bad ? kCritIrregular : x.x, x.y, x.z, x.w);
            *reinterpret_cast<uint4*>(o + 4) = y;
        }
    }
    const bool irr_any = __syncthreads_or(irr) != 0;
    double acc[KE][8];
#pragma unroll
    for (int e = 0; e < KE; ++e) {
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[e][q] = 0.0;
    }
    const int64_t stride = (int64_t)nblk * kBlock * VEC;
    auto sweep = [&](auto chk) {
        constexpr bool CHK = decltype(chk)::value;
        for (int64_t j = ((int64_t)blockIdx.x * kBlock + tid) * VEC; j < a.P; j += stride) {
            float sxa[KE][VEC], sxb[KE][VEC];
            int32_t texa[KE][VEC], texb[KE][VEC];
            {
                float sn[VEC];
                loadf<VEC>(a.S + (int64_t)N * a.ld + j, sn);
#pragma unroll
                for (int e = 0; e < KE; ++e) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        sxa[e][v] = sxb[e][v] = sn[v];
                        texa[e][v] = texb[e][v] = N;
                    }
                }
            }
            auto decide = [&](const float (&row)[VEC], int t) {
#pragma unroll
                for (int e = 0; e < KE; ++e) {
                    const uint32_t* w = sh_t + ((size_t)t * KE + e) * 8;
                    const uint4 ta = *reinterpret_cast<const uint4*>(w);
                    if (CHK && __builtin_amdgcn_readfirstlane(ta.x) == kCritIrregular) {
                        const Fit f = fit_given(a.betas[e], t, N);
                        const double ck = a.cK[e][t], K = a.K[e], invK = a.invK[e];
#pragma unroll
                        for (int v = 0; v < VEC; ++v) {
                            const bool ex = (texa[e][v] == N) & exercises(pay_stored(row[v], K, invK, PUT), f);
                            sxa[e][v] = ex ? row[v] : sxa[e][v];
                            texa[e][v] = ex ? t : texa[e][v];
                            const bool exb = (texb[e][v] == N) & exercises(pay_partner(ck, row[v], K, PUT), f);
                            sxb[e][v] = exb ? row[v] : sxb[e][v];
                            texb[e][v] = exb ? t : texb[e][v];
                        }
                        continue;
                    }
                    const uint4 tb = *reinterpret_cast<const uint4*>(w + 4);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const uint32_t bits = __float_as_uint(row[v]);
                        const bool ex = (texa[e][v] == N) & crit_in(ta, bits);
                        sxa[e][v] = ex ? row[v] : sxa[e][v];
                        texa[e][v] = ex ? t : texa[e][v];
                        const bool exb = (texb[e][v] == N) & crit_in(tb, bits);
                        sxb[e][v] = exb ? row[v] : sxb[e][v];
                        texb[e][v] = exb ? t : texb[e][v];
                    }
                }
            };
            auto live = [&]() {
                bool l = false;
#pragma unroll
                for (int e = 0; e < KE; ++e) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) l |= (texa[e][v] == N) | (texb[e][v] == N);
                }
                return l;
            };
            walk_rows<VEC, true>(a.S + j, a.ld, N, decide, live);
#pragma unroll
            for (int e = 0; e < KE; ++e) {
                const double K = a.K[e];
                const double* cKe = a.cK[e];
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    add_cash_flow(acc[e], payoff_d(sxa[e][v], K, PUT), a.D[texa[e][v] - 1], texa[e][v] < N);
                    add_cash_flow(acc[e], pay_partner(cKe[texb[e][v]], sxb[e][v], K, PUT).imm, a.D[texb[e][v] - 1],
                                  texb[e][v] < N);
                }
            }
        }
    };
    if (irr_any) sweep(std::true_type{});
    else sweep(std::false_type{});
#pragma unroll
    for (int e = 0; e < KE; ++e) {
        if (e) __syncthreads();  // two uses of `red`
        const double s = block_reduce8(acc[e], red);
        if (tid < 64 && (tid & 7) == 0) a.part[e][(size_t)(tid >> 3) * pstride + blockIdx.x] = s;
    }
}

// ------------------------------------------------------------------ host launchers
// LDS of one pass-2 workgroup: the reduction patch plus 32 bytes per step and entry.  A workgroup may take up to 160 KB on
// gfx950, but the walk is a chain of dependent row decisions that needs several workgroups per CU to hide its loads: the
// width stays where at least two fit.
// kChainLdsBudget is the whole workgroup's; the tables get it less the 16.8 KB reduction patch, i.e. 55 KB.
constexpr size_t kChainLdsBudget = 72 * 1024;

int chain_fused_width(const LsmProblem& p)
{
    if (!p.fold_cK || p.N < 2) return 0;
    const FoldGeometry geo = lsm_fold_geometry(p);
    const size_t per_entry = sizeof(uint32_t) * 8 * (size_t)(p.N + 1);
    int w = kChainWidthMax;
    // (registers: 4 x columns-per-thread state words and 16 accumulator registers per entry; beyond 8 entry-columns per
    //  thread the kernel spills to memory -- DESIGN.md section 13.3)
    while (w > 1 && (w * geo.vec2 > 8 || (size_t)w * per_entry > kChainLdsBudget - sizeof(double) * kNQ * kRedStride)) w /= 2;
    if ((size_t)w * per_entry > kChainLdsBudget - sizeof(double) * kNQ * kRedStride) return 0;
    return w;
}

hipError_t chain_pass1_sweep(hipStream_t st, const ChainSweepArgs& a, const LsmProblem& p, int64_t* ntiles)
{
    const Pass1Geometry g = lsm_fold_geometry(p).p1;
    *ntiles = g.ntiles;
    if (p.N < 2 || a.KE < 1 || a.KE > kChainWidthMax) return hipErrorInvalidValue;
    for_vec4(g.v4, [&](auto vec) {
        for_put(a.is_put, [&](auto put) {
            constexpr int VEC = decltype(vec)::value, PUT = decltype(put)::value;
            hipLaunchKernelGGL((lsm_pass1_fold_chain_kernel<VEC, kFoldTpw, PUT>), g.grid, dim3(kBlock), 0, st, a, g.ntiles, g.tchunk);
        });
    });
    return hipGetLastError();
}

template <int VEC, int PUT, int KE>
static hipError_t launch_pass2_chain(hipStream_t st, const ChainSweepArgs& a, int nblk, size_t dyn)
{
    static std::atomic<uint64_t> lds_set{0};
    if (dyn > 32 * 1024) {
        const hipError_t e = set_max_dynamic_lds(lds_set, (const void*)lsm_pass2_fold_chain_kernel<VEC, PUT, KE>,
                                                 kChainLdsBudget - sizeof(double) * kNQ * kRedStride);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((lsm_pass2_fold_chain_kernel<VEC, PUT, KE>), dim3(nblk), dim3(kBlock), dyn, st, a, nblk, kPStride);
    return hipGetLastError();
}

hipError_t chain_pass2_sweep(hipStream_t st, const ChainSweepArgs& a, const LsmProblem& p, int* nblk)
{
    const FoldGeometry geo = lsm_fold_geometry(p);
    *nblk = geo.nblk;
    const size_t dyn = sizeof(uint32_t) * 8 * (size_t)(p.N + 1) * (size_t)a.KE;
    if (dyn > kChainLdsBudget - sizeof(double) * kNQ * kRedStride) return hipErrorInvalidValue;
    if (a.KE != 1 && a.KE != 2 && a.KE != 4) return hipErrorInvalidValue;
    return for_vec(geo.vec2, [&](auto vec) {
        return for_put(a.is_put, [&](auto put) {
            return for_int<1, 2, 4>(a.KE, [&](auto ke) {
                constexpr int VEC = decltype(vec)::value, PUT = decltype(put)::value, KE = decltype(ke)::value;
                // (four entries at four columns per thread would spill: chain_fused_width never asks for them)
                if constexpr (VEC <= 2 || KE < 4) return launch_pass2_chain<VEC, PUT, KE>(st, a, geo.nblk, dyn);
                else return hipErrorInvalidValue;
            });
        });
    });
}

}  // namespace omc
