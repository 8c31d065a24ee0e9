// omc_lsm.hip -- Longstaff-Schwartz backward induction kernels for gfx950 (MI355X).
//
// Replaces the reference's per-step torch/numpy chains (mask -> gather -> regress ->
// compare -> scatter, with host syncs every step):
//   per-step flow   Options_model.py:108-157, options_model_2.py:278-313
//   two-pass flow   options_model_3/options_model_3.py:482-516 (pass 1), :615-651 (pass 2)
//   GPU intent      options_model_3/option_model_3_gpu.py:705-721, :804-831
// The regressor is OLS on [1,u,u^2], u = S/K - 1: eight double sums per time step, reduced
// per block through LDS, solved on chip; nothing is gathered, compacted or materialised.
//
// Per-path state is (sx, tex) = spot and step index of the path's current exercise time
// (tex == N: terminal payoff).  A cash-flow seen from step t is payoff(sx) * D[tex - t]
// with D[k] = exp(-r dt k): no per-step rescaling pass, no rounding drift, and the state is
// only rewritten when a path actually exercises.
//
// All kernels: 256-thread workgroups, 16-byte loads per lane where alignment allows,
// fixed-order reductions (bitwise reproducible), no atomics.
#include "omc_lsm_dev.h"

#include <cstdlib>
#include <cstring>

namespace omc {

// ------------------------------------------------------------------ __global__ entry points
template <int SEM, int VEC, int BLOCK>
__global__ __launch_bounds__(BLOCK) void lsm_step_kernel(StepArgs a)
{
    lsm_step_body<SEM, VEC, BLOCK>(a, blockIdx.x, a.nblk);
}

// the same with the argument block in device memory: the N launches of one sweep differ only in `t`,
// so a captured HIP graph of them can be replayed for any pricing of the same geometry after
// refreshing that block
template <int SEM, int VEC, int BLOCK>
__global__ __launch_bounds__(BLOCK) void lsm_step_ind_kernel(const StepArgs* __restrict__ ap, int t)
{
    StepArgs a = *ap;
    a.t = t;
    lsm_step_body<SEM, VEC, BLOCK>(a, blockIdx.x, a.nblk);
}

__global__ __launch_bounds__(kBlock) void lsm_reduce_step_kernel(const double* part, double* gmom, int t,
                                                                 int nblk, int pstride, int gstride)
{
    lsm_reduce_step_body(part, gmom, t, nblk, pstride, gstride);
}

template <int VEC, int TPW, int PUT>
__global__ __launch_bounds__(kBlock) void lsm_pass1_kernel(Pass1Args a) { lsm_pass1_body<VEC, TPW, PUT>(a); }

__global__ __launch_bounds__(kBlock) void lsm_reduce_pass1_kernel(const double* part1, double* gmom,
                                                                  int64_t ntiles, int N)
{
    lsm_reduce_pass1_body(part1, gmom, ntiles, N);
}

__global__ void lsm_solve_betas_kernel(const double* __restrict__ gmom, double* __restrict__ betas, int N)
{
    lsm_solve_all_body(gmom, betas, N);
}

template <int VEC, bool WRITE_STATE>
__global__ __launch_bounds__(kBlock) void lsm_pass2_kernel(Pass2Args a) { lsm_pass2_body<VEC, WRITE_STATE>(a); }

// the two sweeps on the antithetic-folded matrix (omc_lsm_dev.h)
template <int VEC, int TPW, int PUT>
__global__ __launch_bounds__(kBlock) void lsm_pass1_fold_kernel(Pass1Args a) { lsm_pass1_fold_body<VEC, TPW, PUT>(a); }
template <int VEC, int PUT, bool TAB>
__global__ __launch_bounds__(kBlock) void lsm_pass2_fold_kernel(Pass2Args a) { lsm_pass2_fold_body<VEC, PUT, TAB>(a); }

// pass 2's per-step exercise tables: one workgroup per step t = 0 .. N, a wave per path kind (omc_crit.h)
__global__ __launch_bounds__(128) void lsm_crit_build_kernel(CritArgs a) { lsm_crit_build_body(a); }
__global__ __launch_bounds__(kBlock) void lsm_crit_check_kernel(const uint32_t* tab, const double* betas, const double* cK,
                                                                int N, int is_put, double K, double invK,
                                                                unsigned long long* mism)
{
    lsm_crit_check_body(tab, betas, cK, N, is_put, K, invK, mism);
}

// cK[t] = c0 g^t, t = 0 .. N (fold_table_fill)
__global__ void lsm_fold_table_kernel(double* __restrict__ cK, int N, double c0, double g)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) fold_table_fill(cK, N, c0, g);
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void lsm_final_kernel(FinalArgs a) { lsm_final_body<VEC>(a); }

template <int VEC>
__global__ __launch_bounds__(kBlock) void lsm_final_ind_kernel(const FinalArgs* __restrict__ ap)
{
    lsm_final_body<VEC>(*ap);
}

__global__ __launch_bounds__(kBlock) void lsm_finalize_kernel(const double* part, const double* gmom,
                                                              double* result, int nblk, int N, int pstride)
{
    lsm_finalize_body(part, gmom, result, nblk, N, pstride);
}

struct FinalizeArgs {
    const double* part;
    const double* gmom;
    double* result;
    int nblk, N, pstride, gstride;
};
// device-resident argument block of a captured per-step sweep
struct SweepArgs {
    StepArgs step;
    FinalArgs fin;
    FinalizeArgs fz;
};

__global__ __launch_bounds__(kBlock) void lsm_finalize_ind_kernel(const FinalizeArgs* __restrict__ ap)
{
    const FinalizeArgs a = *ap;
    lsm_finalize_body(a.part, a.gmom, a.result, a.nblk, a.N, a.pstride, a.gstride);
}

// ---- K pricings of one geometry advanced by ONE launch per time step (omc_price_american_seq, per-step flows).
// `tab[k]` holds pricing k's arguments; the chip's workgroups are dealt G per pricing (pricing = blockIdx.x / G),
// so all K pricings are resident together and workgroup w of a pricing walks the slots w, w + G, ... of the
// single-pricing geometry (lsm_step_body): per pricing the bits of its own launch, per launch K x the bytes.
template <int SEM, int VEC, int BLOCK>
__global__ __launch_bounds__(BLOCK) void lsm_step_multi_kernel(const SweepArgs* __restrict__ tab, int G, int t)
{
    const int k = (int)blockIdx.x / G;
    StepArgs a = tab[k].step;
    a.t = t;
    lsm_step_body<SEM, VEC, BLOCK>(a, (int)blockIdx.x - k * G, G);
}

__global__ __launch_bounds__(kBlock) void lsm_reduce_step_multi_kernel(const SweepArgs* __restrict__ tab, int t)
{
    const StepArgs& a = tab[blockIdx.x].step;
    lsm_reduce_step_body(a.part, a.gmom, t, a.nblk, a.pstride, a.gstride);
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void lsm_final_multi_kernel(const SweepArgs* __restrict__ tab)
{
    lsm_final_body<VEC>(tab[blockIdx.z].fin);
}

__global__ __launch_bounds__(kBlock) void lsm_finalize_multi_kernel(const SweepArgs* __restrict__ tab)
{
    const FinalizeArgs a = tab[blockIdx.x].fz;
    lsm_finalize_body(a.part, a.gmom, a.result, a.nblk, a.N, a.pstride, a.gstride);
}

// ---- the two-pass flow's small launches for K pricings of one geometry (omc_price_american_seq): pricing = blockIdx.y,
// its pointers from the by-value argument block; blockIdx.x is what the single launch's body expects.
__global__ __launch_bounds__(kBlock) void lsm_reduce_pass1_group_kernel(SeqGroupArgs g)
{
    const SeqGroupSlot& s = g.slot[blockIdx.y];
    lsm_reduce_pass1_body(s.part1, s.gmom, g.ntiles, s.N);
}

__global__ __launch_bounds__(128) void lsm_crit_build_group_kernel(SeqGroupArgs g)
{
    const SeqGroupSlot& s = g.slot[blockIdx.y];
    if ((int)blockIdx.x > s.N) return;  // (the grid is sized for the longest member)
    CritArgs a;
    a.gmom = s.gmom; a.betas = s.betas; a.betas_out = s.betas; a.cK = s.cK; a.tab = s.crit;
    a.N = s.N; a.is_put = s.is_put; a.K = s.K; a.invK = s.invK; a.irr_every = g.irr_every;
    lsm_crit_build_body(a);
}

__global__ __launch_bounds__(kBlock) void lsm_finalize_group_kernel(SeqGroupArgs g)
{
    const SeqGroupSlot& s = g.slot[blockIdx.y];
    lsm_finalize_body(s.part, s.gmom, s.result, g.nblk, s.N, kPStride);
}

// ------------------------------------------------------------------ host launchers
int lsm_step_blocks(int64_t M)
{
    const int64_t per_block = (int64_t)kBlock * 4;
    int64_t b = (M + per_block - 1) / per_block;
    if (b < 1) b = 1;
    return (int)(b > kMaxLsmBlocks ? kMaxLsmBlocks : b);
}

int lsm_sweep_blocks(int64_t M)
{
    const int64_t per_block = (int64_t)kStepThreads * 4;
    int64_t b = (M + per_block - 1) / per_block;
    if (b < 1) b = 1;
    return (int)(b > kStepMaxBlocks ? kStepMaxBlocks : b);
}

size_t lsm_part1_tiles(int64_t M)
{
    // sized for the VEC=1 fallback too (4x more tiles); the kernel uses what it needs
    return (size_t)((M + kBlock - 1) / kBlock);
}

// ---- the argument blocks (declared in omc_lsm_dev.h)
// the view of the contract that StepArgs, Pass1Args and Pass2Args share
template <class Args>
static void set_contract(Args& a, const LsmProblem& p, const LsmWorkspace& w)
{
    a.S = p.S; a.ld = p.ld; a.M = p.M; a.N = p.N; a.is_put = p.is_put;
    a.K = p.K; a.invK = 1.0 / p.K; a.D = w.D;
}

StepArgs step_args(const LsmProblem& p, const LsmWorkspace& w, int t, bool external_moments)
{
    StepArgs a{};
    set_contract(a, p, w);
    a.sx = w.sx; a.tex = w.tex; a.live = w.live; a.part = w.part; a.gmom = w.gmom; a.betas = w.betas;
    a.t = t; a.nblk = lsm_sweep_blocks(p.M); a.external = external_moments ? 1 : 0;
    a.pstride = kPStride;
    a.gstride = w.gstride;
    a.cont = w.cont; a.ldc = w.ldc;
    return a;
}

Pass1Args pass1_args(const LsmProblem& p, const LsmWorkspace& w, int64_t ntiles, int tchunk)
{
    Pass1Args a{};
    set_contract(a, p, w);
    a.part1 = w.part1; a.ntiles = ntiles; a.tchunk = tchunk;
    if (p.fold_cK) {  // the folded matrix: M / 2 stored columns
        a.M = p.M / 2;
        a.cK = p.fold_cK;
    }
    return a;
}

Pass2Args pass2_args(const LsmProblem& p, const LsmWorkspace& w, int nblk)
{
    Pass2Args a{};
    set_contract(a, p, w);
    a.betas = w.betas; a.sx = w.sx; a.tex = w.tex; a.part = w.part;
    a.nblk = nblk; a.pstride = kPStride;
    if (p.fold_cK) {  // the folded matrix: M / 2 stored columns, both partners decided from every spot; no state arrays
        a.M = p.M / 2;
        a.cK = p.fold_cK;
    }
    return a;
}

FinalArgs final_args(const LsmProblem& p, const LsmWorkspace& w, int tval, bool use_flags, bool fill_state)
{
    FinalArgs a{};
    a.sx = w.sx; a.tex = w.tex; a.live = use_flags ? w.live : nullptr;
    a.M = p.M; a.N = p.N; a.is_put = p.is_put; a.tval = tval; a.fill_state = fill_state ? 1 : 0;
    a.K = p.K; a.D = w.D; a.part = w.part;
    a.nblk = lsm_step_blocks(p.M); a.pstride = kPStride;
    return a;
}

// `ind` != null: the kernel reads its arguments from that device block (see lsm_step_args)
static hipError_t lsm_step_impl(hipStream_t st, const LsmProblem& p, const LsmWorkspace& w, int semantics,
                                int t, bool external_moments, const StepArgs* ind)
{
    const StepArgs a = step_args(p, w, t, external_moments);
    const size_t dyn = semantics == 1 ? sizeof(double) * (size_t)(p.N + 1) : 0;
    for_step(semantics, rows_aligned(4, p.M, p.S, p.ld), [&](auto sem, auto vec, auto block) {
        constexpr int SEM = decltype(sem)::value, VEC = decltype(vec)::value, BLOCK = decltype(block)::value;
        const dim3 grid(a.nblk), threads(BLOCK);
        if (ind) hipLaunchKernelGGL((lsm_step_ind_kernel<SEM, VEC, BLOCK>), grid, threads, dyn, st, ind, t);
        else hipLaunchKernelGGL((lsm_step_kernel<SEM, VEC, BLOCK>), grid, threads, dyn, st, a);
    });
    return hipGetLastError();
}

hipError_t lsm_step(hipStream_t st, const LsmProblem& p, const LsmWorkspace& w, int semantics,
                    int t, bool external_moments)
{
    return lsm_step_impl(st, p, w, semantics, t, external_moments, nullptr);
}

size_t lsm_sweep_args_bytes() { return sizeof(SweepArgs); }

// host image of the device argument block the indirect kernels read
void lsm_sweep_args_image(const LsmProblem& p, const LsmWorkspace& w, int semantics, bool fill_state, void* out,
                          bool external_moments)
{
    SweepArgs s;
    memset(&s, 0, sizeof s);
    s.step = step_args(p, w, 0, external_moments);
    s.fin = final_args(p, w, semantics == 1 ? 0 : 1, semantics == 0, fill_state);
    s.fz.part = w.part; s.fz.gmom = w.gmom; s.fz.result = w.result;
    s.fz.nblk = s.fin.nblk; s.fz.N = p.N; s.fz.pstride = kPStride; s.fz.gstride = w.gstride;
    memcpy(out, &s, sizeof s);
}

// workgroups per pricing when K pricings share the launches of a per-step sweep: the chip's workgroups (one
// 1024-thread workgroup per CU) divided by K, at least what keeps a workgroup within kStepMaxItems slots
int lsm_multi_groups(int64_t M, int K, int device_cus)
{
    const int nblk = lsm_sweep_blocks(M);
    const int wgs = device_cus > 0 ? device_cus : 256;
    int G = wgs / (K > 0 ? K : 1);
    const int gmin = (nblk + kStepMaxItems - 1) / kStepMaxItems;
    if (G < gmin) G = gmin;
    if (G < 1) G = 1;
    return G > nblk ? nblk : G;
}

hipError_t lsm_step_multi(hipStream_t st, const void* table_dev, int K, int G, int semantics, bool vec4, int N, int t)
{
    const SweepArgs* tab = (const SweepArgs*)table_dev;
    const dim3 grid((unsigned)(K * G));
    const size_t dyn = semantics == 1 ? sizeof(double) * (size_t)(N + 1) : 0;
    for_step(semantics, vec4, [&](auto sem, auto vec, auto block) {
        constexpr int SEM = decltype(sem)::value, VEC = decltype(vec)::value, BLOCK = decltype(block)::value;
        hipLaunchKernelGGL((lsm_step_multi_kernel<SEM, VEC, BLOCK>), grid, dim3(BLOCK), dyn, st, tab, G, t);
    });
    return hipGetLastError();
}

hipError_t lsm_reduce_step_moments_multi(hipStream_t st, const void* table_dev, int K, int t)
{
    hipLaunchKernelGGL(lsm_reduce_step_multi_kernel, dim3(K), dim3(kBlock), 0, st, (const SweepArgs*)table_dev, t);
    return hipGetLastError();
}

// valuation + finalize of all K pricings: two launches
hipError_t lsm_final_multi(hipStream_t st, const void* table_dev, int K, int64_t M)
{
    const SweepArgs* tab = (const SweepArgs*)table_dev;
    const int nblk = lsm_step_blocks(M);
    for_vec4(state_vec4(M), [&](auto vec) {
        hipLaunchKernelGGL((lsm_final_multi_kernel<decltype(vec)::value>), dim3(nblk, 1, K), dim3(kBlock), 0, st, tab);
    });
    hipLaunchKernelGGL(lsm_finalize_multi_kernel, dim3(K), dim3(kBlock), 0, st, tab);
    return hipGetLastError();
}

// the whole per-step sweep (N step launches + valuation + finalize) with device-resident arguments:
// this is what gets captured into a HIP graph.  Launch geometry depends on (M, N, semantics, ld, S
// alignment) only -- the graph's cache key.
hipError_t lsm_sweep_indirect(hipStream_t st, const LsmProblem& p, const LsmWorkspace& w, int semantics,
                              const void* args_dev)
{
    const SweepArgs* sa = (const SweepArgs*)args_dev;
    for (int t = p.N; t >= 1; --t) {
        hipError_t e = lsm_step_impl(st, p, w, semantics, t, false, &sa->step);
        if (e != hipSuccess) return e;
    }
    const int nblk = lsm_step_blocks(p.M);
    for_vec4(state_vec4(p.M), [&](auto vec) {
        hipLaunchKernelGGL((lsm_final_ind_kernel<decltype(vec)::value>), dim3(nblk), dim3(kBlock), 0, st, &sa->fin);
    });
    hipLaunchKernelGGL(lsm_finalize_ind_kernel, dim3(1), dim3(kBlock), 0, st, &sa->fz);
    return hipGetLastError();
}

hipError_t lsm_reduce_step_moments(hipStream_t st, const LsmWorkspace& w, int t, int nblk)
{
    hipLaunchKernelGGL(lsm_reduce_step_kernel, dim3(1), dim3(kBlock), 0, st, w.part, w.gmom, t, nblk,
                       kPStride, w.gstride);
    return hipGetLastError();
}

hipError_t lsm_fold_table(hipStream_t st, double* cK, int N, double c0, double g)
{
    hipLaunchKernelGGL(lsm_fold_table_kernel, dim3(1), dim3(64), 0, st, cK, N, c0, g);
    return hipGetLastError();
}

// steps per workgroup of a pass-1 sweep: `tchunk`, or what OMC_PASS1_TCHUNK asks for when that is 2 .. max (the only
// tuning knob left: tools/soak_tchunk.py walks the chunk lengths with it)
static int pass1_tchunk(int tchunk, int max)
{
    static const int env = getenv("OMC_PASS1_TCHUNK") ? atoi(getenv("OMC_PASS1_TCHUNK")) : 0;
    return (env >= 2 && env <= max) ? env : tchunk;
}

static dim3 pass1_grid(int64_t ntiles, int N, int tchunk)
{
    return dim3((unsigned)((ntiles + 3) / 4), (unsigned)((N - 1 + tchunk - 1) / tchunk));
}

// The launch geometry of pass 1 on the full matrix of `p`: kPass1Tpw tiles of 64 x VEC columns per wave and step
// (defaults measured on MI355X)
Pass1Geometry lsm_pass1_geometry(const LsmProblem& p)
{
    Pass1Geometry g;
    g.v4 = rows_aligned(4, p.M, p.S, p.ld);
    const int64_t per_wave = 64 * (int64_t)(g.v4 ? 4 : 1) * kPass1Tpw;  // paths per wave per step
    g.ntiles = (p.M + per_wave - 1) / per_wave;
    // Steps per workgroup.  The kernel holds 3 waves per SIMD (152 VGPRs), i.e. 3 workgroups per CU: when all the
    // workgroups of a launch fit on the chip at once there is no partly filled last round of dispatch (measured at
    // C2, 245 tile-workgroups: 8 chunks of 32 steps = 2.55 rounds 0.214 ms, 4 x 63 = 1.28 rounds 0.230, 3 x 84 =
    // 0.96 round 0.207), so take the most chunks that still fit; larger problems run many rounds and keep 32.
    // The partition changes no sum: partials are per (step, tile).
    static const int cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            n = 256;
        return n > 0 ? n : 256;
    }();
    int tchunk = 32;
    const int64_t wgs_x = (g.ntiles + 3) / 4;
    if (wgs_x <= 3 * (int64_t)cus && p.N > 2) {
        const int chunks = (int)((3 * (int64_t)cus) / wgs_x);
        const int t = (p.N - 1 + chunks - 1) / chunks;
        if (t <= 126 && t >= 32) tchunk = t;
    }
    g.tchunk = pass1_tchunk(tchunk, kPass1MaxChunk);
    g.grid = pass1_grid(g.ntiles, p.N, g.tchunk);
    return g;
}

// The launch geometry of the two sweeps on the folded matrix of `p` (declared in omc_kernels.h: the chain sweeps of
// omc_chain.hip form their sums in the very same tiles, blocks and slots).  Pass 1: P = M / 2 stored columns, kFoldTpw
// tiles of 64 x VEC columns per wave and step (= 1,024 paths, as in the full sweep).
FoldGeometry lsm_fold_geometry(const LsmProblem& p)
{
    FoldGeometry g;
    const int64_t P = p.M / 2;
    g.p1.v4 = rows_aligned(4, P, p.S, p.ld);
    const int64_t per_wave = 64 * (int64_t)(g.p1.v4 ? 4 : 1) * kFoldTpw;
    g.p1.ntiles = (P + per_wave - 1) / per_wave;
    // Steps per workgroup: the folded sweep is bound by its float64 arithmetic, not by the rows it reads, so what counts is
    // that every CU stays busy to the end -- many short workgroups (measured at C2, 245 tile-workgroups: chunks of 16-32
    // steps 0.145-0.147 ms, 63 steps 0.156, 84 steps -- one resident round -- 0.162, 126 steps 0.183; 8M paths: 32).
    g.p1.tchunk = pass1_tchunk(32, kFoldMaxChunk);
    g.p1.grid = pass1_grid(g.p1.ntiles, p.N, g.p1.tchunk);
    // columns per thread of the folded pass 2: 2 (8-byte loads, twice the threads) until the 16-byte form alone fills the
    // chip with workgroups (measured: C2's 0.5M columns 0.131 against 0.136 ms, C3's 4M columns 1.026 against 1.008)
    g.fvec = P >= (int64_t(1) << 21) ? 4 : 2;
    g.nblk = lsm_step_blocks(P * (4 / g.fvec));
    g.vec2 = g.p1.v4 ? g.fvec : 1;
    return g;
}

// pass 1, full or folded storage: geometry, arguments, dispatch
hipError_t lsm_pass1_sweep(hipStream_t st, const LsmProblem& p, const LsmWorkspace& w, int64_t* ntiles)
{
    *ntiles = 0;
    if (p.N < 2) return hipSuccess;
    const Pass1Geometry g = p.fold_cK ? lsm_fold_geometry(p).p1 : lsm_pass1_geometry(p);
    const Pass1Args a = pass1_args(p, w, g.ntiles, g.tchunk);
    if (w.ev_p1_begin) (void)hipEventRecord(w.ev_p1_begin, st);
    for_flag(p.fold_cK != nullptr, [&](auto fold) {
        for_vec4(g.v4, [&](auto vec) {
            for_put(p.is_put, [&](auto put) {
                constexpr int VEC = decltype(vec)::value, PUT = decltype(put)::value;
                if constexpr (decltype(fold)::value)
                    hipLaunchKernelGGL((lsm_pass1_fold_kernel<VEC, kFoldTpw, PUT>), g.grid, dim3(kBlock), 0, st, a);
                else hipLaunchKernelGGL((lsm_pass1_kernel<VEC, kPass1Tpw, PUT>), g.grid, dim3(kBlock), 0, st, a);
            });
        });
    });
    if (w.ev_p1_end) (void)hipEventRecord(w.ev_p1_end, st);
    *ntiles = a.ntiles;
    return hipGetLastError();
}

hipError_t lsm_reduce_pass1(hipStream_t st, const LsmWorkspace& w, int64_t ntiles, int N)
{
    if (N < 2) return hipSuccess;
    hipLaunchKernelGGL(lsm_reduce_pass1_kernel, dim3(N - 1), dim3(kBlock), 0, st, w.part1, w.gmom, ntiles, N);
    return hipGetLastError();
}

hipError_t lsm_pass1_moments(hipStream_t st, const LsmProblem& p, const LsmWorkspace& w)
{
    int64_t ntiles = 0;
    const hipError_t e = lsm_pass1_sweep(st, p, w, &ntiles);
    return e != hipSuccess ? e : lsm_reduce_pass1(st, w, ntiles, p.N);
}

// exercise tables (option "pass2_tables"): built from the fits right before the sweep, which then reads the fits
// the table kernel solved (or was given) from w.betas instead of solving all N in every workgroup
bool lsm_pass2_tables(const LsmProblem& p, const LsmWorkspace& w, bool write_state)
{
    return w.crit != nullptr && p.fold_cK != nullptr && !write_state;
}

hipError_t lsm_pass2_sweep(hipStream_t st, const LsmProblem& p, const LsmWorkspace& w, bool write_state,
                           bool solve_from_moments, int* nblk_out)
{
    const bool fold = p.fold_cK != nullptr;
    const FoldGeometry geo = fold ? lsm_fold_geometry(p) : FoldGeometry{};
    const int nblk = fold ? geo.nblk : lsm_step_blocks(p.M);
    *nblk_out = nblk;
    if (fold && write_state) return hipErrorInvalidValue;  // (the folded sweep keeps no state arrays)
    Pass2Args a = pass2_args(p, w, nblk);
    const bool tab = lsm_pass2_tables(p, w, write_state);
    if (tab) {  // the table launch solved the fits into w.betas
        a.crit = w.crit;
    } else if (solve_from_moments) {
        a.gmom = w.gmom;
        a.betas_out = w.betas;
    }
    const size_t dyn = sizeof(double) * 4 * (size_t)(p.N + 1);
    const dim3 grid(nblk), block(kBlock);
    if (fold) {
        for_vec(geo.vec2, [&](auto vec) {
            for_put(p.is_put, [&](auto put) {
                for_flag(tab, [&](auto tb) {
                    constexpr int VEC = decltype(vec)::value, PUT = decltype(put)::value;
                    hipLaunchKernelGGL((lsm_pass2_fold_kernel<VEC, PUT, decltype(tb)::value>), grid, block, dyn, st, a);
                });
            });
        });
    } else {
        for_vec4(rows_aligned(4, p.M, p.S, p.ld), [&](auto vec) {
            for_flag(write_state, [&](auto ws) {
                hipLaunchKernelGGL((lsm_pass2_kernel<decltype(vec)::value, decltype(ws)::value>), grid, block, dyn, st, a);
            });
        });
    }
    if (w.ev_p2_end) (void)hipEventRecord(w.ev_p2_end, st);
    return hipGetLastError();
}

hipError_t lsm_pass2_apply(hipStream_t st, const LsmProblem& p, const LsmWorkspace& w,
                           bool write_state, bool solve_from_moments)
{
    if (w.ev_p2_begin) (void)hipEventRecord(w.ev_p2_begin, st);
    const bool tab = lsm_pass2_tables(p, w, write_state);
    if (tab) {
        CritArgs c;
        c.gmom = solve_from_moments ? w.gmom : nullptr; c.betas = w.betas; c.betas_out = solve_from_moments ? w.betas : nullptr;
        c.cK = p.fold_cK; c.tab = w.crit;
        c.N = p.N; c.is_put = p.is_put; c.K = p.K; c.irr_every = w.crit_irr_every;
        const hipError_t e = lsm_crit_build(st, c);
        if (e != hipSuccess) return e;
    }
    int nblk = 0;
    const hipError_t e = lsm_pass2_sweep(st, p, w, write_state, solve_from_moments, &nblk);
    return e != hipSuccess ? e : lsm_finalize(st, w.part, w.gmom, w.result, nblk, p.N);
}

SeqGroupSlot lsm_group_slot(const LsmProblem& p, const LsmWorkspace& w)
{
    SeqGroupSlot s;
    s.part1 = w.part1; s.gmom = w.gmom; s.betas = w.betas; s.crit = w.crit; s.part = w.part; s.result = w.result;
    s.cK = p.fold_cK;
    s.K = p.K; s.invK = 1.0 / p.K; s.is_put = p.is_put; s.N = p.N;
    return s;
}

hipError_t lsm_group_reduce_pass1(hipStream_t st, const SeqGroupArgs& g, int K)
{
    if (g.N < 2) return hipSuccess;
    hipLaunchKernelGGL(lsm_reduce_pass1_group_kernel, dim3(g.N - 1, K), dim3(kBlock), 0, st, g);
    return hipGetLastError();
}

hipError_t lsm_group_crit_build(hipStream_t st, const SeqGroupArgs& g, int K)
{
    hipLaunchKernelGGL(lsm_crit_build_group_kernel, dim3(g.N + 1, K), dim3(128), 0, st, g);
    return hipGetLastError();
}

hipError_t lsm_group_finalize(hipStream_t st, const SeqGroupArgs& g, int K)
{
    hipLaunchKernelGGL(lsm_finalize_group_kernel, dim3(1, K), dim3(kBlock), 0, st, g);
    return hipGetLastError();
}

hipError_t lsm_crit_build(hipStream_t st, CritArgs c)
{
    c.invK = 1.0 / c.K;
    hipLaunchKernelGGL(lsm_crit_build_kernel, dim3(c.N + 1), dim3(128), 0, st, c);
    return hipGetLastError();
}

hipError_t lsm_crit_check(hipStream_t st, const double* betas, const double* cK, uint32_t* tab, int N, int is_put,
                          double K, int irr_every, unsigned long long* mism)
{
    CritArgs c;
    c.betas = betas; c.cK = cK; c.tab = tab; c.N = N; c.is_put = is_put; c.K = K; c.irr_every = irr_every;
    const hipError_t e = lsm_crit_build(st, c);
    if (e != hipSuccess || N < 2) return e;
    hipLaunchKernelGGL(lsm_crit_check_kernel, dim3(2048, N - 1), dim3(kBlock), 0, st, tab, betas, cK, N, is_put, K,
                       1.0 / K, mism);
    return hipGetLastError();
}

hipError_t lsm_solve_betas(hipStream_t st, const double* gmom, double* betas, int N)
{
    if (N < 2) return hipSuccess;
    hipLaunchKernelGGL(lsm_solve_betas_kernel, dim3((N + kBlock - 1) / kBlock), dim3(kBlock), 0, st, gmom, betas, N);
    return hipGetLastError();
}

hipError_t lsm_finalize(hipStream_t st, const double* part, const double* gmom, double* result,
                        int nblk, int N)
{
    hipLaunchKernelGGL(lsm_finalize_kernel, dim3(1), dim3(kBlock), 0, st, part, gmom, result, nblk, N,
                       kPStride);
    return hipGetLastError();
}

hipError_t lsm_final_reduce(hipStream_t st, const LsmProblem& p, const LsmWorkspace& w, int tval, bool use_flags,
                            bool fill_state)
{
    const FinalArgs a = final_args(p, w, tval, use_flags, fill_state);
    for_vec4(state_vec4(p.M), [&](auto vec) {
        hipLaunchKernelGGL((lsm_final_kernel<decltype(vec)::value>), dim3(a.nblk), dim3(kBlock), 0, st, a);
    });
    return lsm_finalize(st, w.part, w.gmom, w.result, a.nblk, p.N);
}

}  // namespace omc
