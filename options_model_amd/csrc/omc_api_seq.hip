// omc_api_seq.hip -- omc_price_american_seq, omc_seq_step_width and omc_seq_group_width (include/omc.h): sequences of
// pricings, overlapped across GPUs, advanced K per launch by the per-step flows, or -- two-pass flow -- in groups of K
// that share their small launches.
#include <cstdlib>

#include "omc_ctx.h"

using namespace omc::abi;

extern "C" {

// The event set of pricing i of a sequence, or nullptr when it carries no kernel timings: the context's own seven events
// for the first pricing, a further set from a pool that grows on demand for every seq_event_stride-th one.
static int pricing_events(omc_ctx* c, int i, hipEvent_t** out)
{
    const int k = c->seq_event_stride, s = i == 0 ? 0 : (k > 0 && i % k == 0) ? i / k : -1;
    *out = s == 0 ? c->ev : nullptr;
    if (s <= 0) return 0;
    while (c->ev_pool.size() < 7 * (size_t)s) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreate(&e));
        c->ev_pool.push_back(e);
    }
    *out = c->ev_pool.data() + 7 * (size_t)(s - 1);
    return 0;
}

// ---- overlapped sequence across GPUs ------------------------------------------------------------------------
// omc_price_american_seq across GPUs, two-pass flow, native communicator: per pricing the only exchange the
// decisions wait for is the all-reduce of the [N+1][8] moment table between pass 1 and the solves.  Left on
// the main stream it idles the GPU for a collective's latency once per pricing; here it runs on its own
// stream while the main stream generates the NEXT pricing's paths into a second path buffer AND runs its pass 1
// (second partial / moment buffers), and the 8 result sums of all n pricings are all-reduced once, at the end.
// Kernel adjacency stays that of a single pricing -- pass 1 right behind its generator (it starts with the
// rows that are still in the Infinity Cache), pass 2 behind a pass 1 (measured: a pass 2 right behind a
// generator of ANOTHER buffer pays that generator's write-back, +55 us).  Same kernels, same order of every
// reduction: results are bit-identical to the one-at-a-time path.
static bool seq_overlap_enabled(const omc_ctx* c)
{
    if (c->seq_overlap >= 0) return c->seq_overlap != 0;
    static const int env = [] {
        const char* e = getenv("OMC_SEQ_OVERLAP");
        return e ? atoi(e) : -1;
    }();
    if (env >= 0) return env != 0;
    // default: off.  The mechanism uses one communicator from two streams; callers switch it on once the job has
    // checked, with its real communicator, that the overlapped sequence returns the sequential one's bits
    // (bench.py does so before anything is timed).  With one rank it only costs its event hand-overs
    // (0.606 against 0.591 ms per pricing at C2).
    return false;
}

static bool seq_can_overlap(const omc_ctx* c, const omc_params* p, int n)
{
    if (!c->comm || n < 2 || !seq_overlap_enabled(c)) return false;
    for (int i = 0; i < n; ++i)
        if (p[i].semantics != OMC_SEM_TWO_PASS || p[i].n_paths != p[0].n_paths || p[i].n_steps != p[0].n_steps ||
            p[i].r != p[0].r || p[i].T != p[0].T || p[i].n_steps < 2)
            return false;
    return true;
}

static int enqueue_seq_overlapped(omc_ctx* c, const omc_params* p, int n, double* out_pin)
{
    int rc;
    const int64_t M = p[0].n_paths;
    const int N = p[0].n_steps;
    const int64_t ld = padded_ld(M);
    const size_t sbytes = sizeof(float) * (size_t)ld * (size_t)(N + 1);
    if ((rc = c->S.ensure(sbytes))) return rc;
    if ((rc = c->S2.ensure(sbytes))) return rc;
    if ((rc = c->seq_local.ensure(sizeof(double) * 8 * (size_t)n))) return rc;
    omc::LsmWorkspace w[2];
    if ((rc = prepare_lsm(c, M, N, p[0].r, p[0].T, true, false, &w[0]))) return rc;
    // second set of the buffers a pricing owns between its pass 1 and its solves
    if ((rc = c->part1b.ensure(sizeof(double) * 8 * (size_t)(N + 1) * (size_t)w[0].part1_tiles))) return rc;
    if ((rc = c->gmomb.ensure(sizeof(double) * 8 * (size_t)(N + 1)))) return rc;
    w[1] = w[0];
    w[1].part1 = (double*)c->part1b.p;
    w[1].gmom = (double*)c->gmomb.p;
    if (!c->comm_stream) HIP_TRY(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) {
        if (!c->ev_moments[b]) HIP_TRY(hipEventCreateWithFlags(&c->ev_moments[b], hipEventDisableTiming));
        if (!c->ev_reduced[b]) HIP_TRY(hipEventCreateWithFlags(&c->ev_reduced[b], hipEventDisableTiming));
    }
    float* Sb[2] = {(float*)c->S.p, (float*)c->S2.p};
    double* local = (double*)c->seq_local.p;
    // every pricing of the sequence chooses its storage for itself (folded matrices are smaller than `sbytes`); the two
    // pricings in flight use different cK tables
    std::vector<int64_t> ldk((size_t)n, ld);
    std::vector<const double*> cKk((size_t)n, nullptr);
    auto problem = [&](int k) {
        omc::LsmProblem q{Sb[k & 1], ldk[(size_t)k], M, N, p[k].is_put ? 1 : 0, p[k].K, p[k].r, p[k].T};
        q.fold_cK = cKk[(size_t)k];
        return q;
    };
    // paths + pass 1 of pricing k on the main stream, then its moment table's all-reduce on the other one
    auto phase_a = [&](int k) -> int {
        const int b = k & 1;
        omc::LsmWorkspace wk = w[b];
        int r2;
        hipEvent_t* evs = nullptr;  // the first pricing (and every seq_event_stride-th) carries timing events
        if ((r2 = pricing_events(c, k, &evs))) return r2;
        if (evs) {
            wk.ev_p1_end = evs[4];
            HIP_TRY(hipEventRecord(evs[0], c->stream));
        }
        if ((r2 = plan_storage(c, &p[k], b, &ldk[(size_t)k], &cKk[(size_t)k]))) return r2;
        if ((r2 = enqueue_paths(c, &p[k], Sb[b], ldk[(size_t)k], cKk[(size_t)k] != nullptr))) return r2;
        if (evs) HIP_TRY(hipEventRecord(evs[1], c->stream));
        HIP_TRY(omc::lsm_pass1_moments(c->stream, problem(k), wk));
        HIP_TRY(hipEventRecord(c->ev_moments[b], c->stream));
        HIP_TRY(hipStreamWaitEvent(c->comm_stream, c->ev_moments[b], 0));
        std::string err;
        if ((r2 = omc::comm_allreduce_f64(c->comm, wk.gmom, (size_t)(8 * (N + 1)), 0, c->comm_stream, &err)))
            return fail(r2, err.c_str());
        HIP_TRY(hipEventRecord(c->ev_reduced[b], c->comm_stream));
        return 0;
    };
    if ((rc = phase_a(0))) return rc;
    for (int k = 0; k < n; ++k) {
        // pricing k+1's paths and pass 1 run while pricing k's collective is in flight
        if (k + 1 < n && (rc = phase_a(k + 1))) return rc;
        const int b = k & 1;
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_reduced[b], 0));
        omc::LsmWorkspace wk = w[b];
        hipEvent_t* evs = nullptr;
        if ((rc = pricing_events(c, k, &evs))) return rc;
        if (evs) { wk.ev_p2_begin = evs[5]; wk.ev_p2_end = evs[6]; }
        wk.result = local + 8 * (size_t)k;
        HIP_TRY(omc::lsm_pass2_apply(c->stream, problem(k), wk, false, true));
        if (evs && k == 0) HIP_TRY(hipEventRecord(evs[2], c->stream));
    }
    if ((rc = allreduce(c, local, 8 * n))) return rc;  // all result sums in one collective
    HIP_TRY(hipMemcpyAsync(out_pin, local, sizeof(double) * 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    return 0;
}

// ---- per-step flows: K pricings of one geometry per launch --------------------------------------------------
// One launch of the per-step kernel moves 13 MB at C2 and costs ~6 us, of which ~3.6 us are the launch boundary
// and the cold start of a new kernel: a single pricing is at its latency floor, the chip
// is not.  A sequence of pricings that share (n_paths, n_steps, r, T, semantics) therefore advances K of them
// with every launch: K path matrices, K sets of state / partials / fits, ONE launch boundary per time step; across
// GPUs the K moment vectors of a step travel in ONE all-reduce of 8K doubles.  Per pricing the arithmetic and
// the order of every sum are those of its own launches (lsm_step_body), so res[i] keeps the bits of
// omc_price_american(p[i]).
// What the sequence itself allows: depends on the pricings, the context's settings and the environment only -- never on
// this card's free memory -- so every rank of a job computes the same number (they are handed the same sequence).
static int seq_multi_ideal(const omc_ctx* c, const omc_params* p, int n)
{
    if (n < 2) return 1;
    static const int env_k = getenv("OMC_SEQ_STEP_K") ? atoi(getenv("OMC_SEQ_STEP_K")) : -1;
    int k = c->seq_step_k >= 0 ? c->seq_step_k : env_k;
    if (k < 0) {
        // default: as many pricings as keep one launch's rows and state within ~200 MB (measured, tools/exp_step_k.py:
        // at 1M paths the pricing rate rises up to 16-20 pricings per launch -- 0.66 of the HBM roofline -- and falls
        // beyond 240 MB per launch; 250k-path pricings still gain at 32), at most 32; problems so large that fewer
        // than 4 fit are bandwidth-bound one at a time already (8M paths: 0.62 alone, 0.59 with 4 per launch)
        const double per = (p[0].semantics == OMC_SEM_REFERENCE ? 12.0 : 16.0) * (double)p[0].n_paths;
        k = (int)(2.0e8 / per);
        if (k > 32) k = 32;
        if (k < 4) k = 1;
    }
    if (k < 2) return 1;
    if (p[0].semantics == OMC_SEM_TWO_PASS || p[0].n_steps < 1) return 1;
    if (step_graph_enabled(c)) return 1;
    for (int i = 1; i < n; ++i)
        if (p[i].semantics != p[0].semantics || p[i].n_paths != p[0].n_paths || p[i].n_steps != p[0].n_steps ||
            p[i].r != p[0].r || p[i].T != p[0].T)
            return 1;
    if (k > n) k = n;
    if (k > 32) k = 32;
    return k < 2 ? 1 : k;
}

// What THIS card has room for (rank-dependent).  K path matrices stay resident: bounded by a byte budget -- at most 64 GB
// of the 288 (OMC_SEQ_STEP_BYTES), and never more than 80 % of what is free on this card right now plus what the context
// already holds for them (a card shared with torch or with other ranks has less; seq_multi_reserve also halves K when
// the allocation fails all the same).
// (`held`: bytes the context already holds for the matrices in question; shared by the two-pass groups below)
static double seq_resident_budget(const omc_ctx* c, size_t held)
{
    static const double cap = getenv("OMC_SEQ_STEP_BYTES") ? atof(getenv("OMC_SEQ_STEP_BYTES")) : 64e9;
    double budget = cap;
    size_t free_b = 0, total_b = 0;
    (void)hipSetDevice(c->device);
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const double avail = 0.8 * (double)free_b + (double)held;
        if (avail < budget) budget = avail;
    } else {
        (void)hipGetLastError();
    }
    return budget;
}

static int seq_multi_fit(const omc_ctx* c, const omc_params* p, int k)
{
    const int64_t ld = padded_ld(p[0].n_paths);
    const double sbytes = 4.0 * (double)ld * (double)(p[0].n_steps + 1);
    const int fit = (int)(seq_resident_budget(c, c->mS.cap) / sbytes);
    if (k > fit) k = fit;
    return k < 2 ? 1 : k;
}

// this rank's own estimate (omc_seq_step_width; a job agrees on the smallest in seq_multi_reserve)
static int seq_multi_width(const omc_ctx* c, const omc_params* p, int n)
{
    const int k = seq_multi_ideal(c, p, n);
    return k < 2 ? 1 : seq_multi_fit(c, p, k);
}

// Device memory of the K-pricings-per-launch sweep (K path matrices + per-pricing state).  -> 0, or the HIP error.
static int seq_multi_alloc(omc_ctx* c, int64_t M, int N, int K)
{
    int rc;
    const int64_t ld = padded_ld(M);
    const size_t sbytes = sizeof(float) * (size_t)ld * (size_t)(N + 1);
    const size_t per = up256(sizeof(float) * (size_t)M) + up256(sizeof(int32_t) * (size_t)M) + up256(sizeof(float) * (size_t)M + 16) +
                       up256(sizeof(double) * 2 * 8 * omc::kMaxLsmBlocks) + up256(sizeof(double) * 4 * (size_t)(N + 1));
    const size_t gbytes = up256(sizeof(double) * 8 * (size_t)K * (size_t)(N + 1));
    if ((rc = c->mS.ensure(sbytes * (size_t)K))) return rc;
    if ((rc = c->mstate.ensure(gbytes + per * (size_t)K))) return rc;
    return c->mtable.ensure(omc::lsm_sweep_args_bytes() * (size_t)K);
}

// Reserve for K pricings per launch; when the card has no room (shared with torch, several ranks on one device, a
// smaller card) halve K down to one pricing at a time instead of failing the sequence.
// Ranks of one job must agree on K (their per-step collectives carry 8K doubles, their direct exchanges K jobs), and a
// rank must never skip a collective its peers enter.  So: whether a vote takes place depends on seq_multi_ideal alone
// (the same on every rank); when it does, EVERY rank votes -- also one whose own K came out as 1, also one whose
// allocation failed for another reason than memory -- through the context's generic all-reduce (communicator or
// hook): a one-hot vector of 33 counters plus an error counter, summed; the job takes the smallest K anybody voted
// for, and fails everywhere if anybody reported an error.
static int seq_multi_reserve(omc_ctx* c, const omc_params* p, int n, int* K_out)
{
    *K_out = 1;
    const int ideal = seq_multi_ideal(c, p, n);
    if (ideal < 2) return 0;  // (every rank takes this branch together)
    int K = seq_multi_fit(c, p, ideal), rc = 0, err = 0;
    std::string err_text;
    while (K >= 2 && (rc = seq_multi_alloc(c, p[0].n_paths, p[0].n_steps, K)) != 0) {
        if (rc != (int)hipErrorOutOfMemory && rc != (int)hipErrorMemoryAllocation) {
            err = rc;
            err_text = g_err;
            break;
        }
        K /= 2;
    }
    if (K < 2 || err) K = 1;
    if (c->distributed()) {
        constexpr int kVote = 34;  // K = 1 .. 32 one-hot (slot K), slot 33 = ranks in trouble
        double vote[kVote] = {0};
        vote[K] = 1.0;
        vote[33] = err ? 1.0 : 0.0;
        if ((rc = c->seq_vote.ensure(sizeof vote))) return rc;  // (never allocates: the buffer exists since the communicator / hook was installed)
        if ((rc = allreduce_host(c, (double*)c->seq_vote.p, vote, kVote))) return rc;
        if (vote[33] > 0.0) {
            if (err) return fail(err, err_text.c_str());
            return fail(3101, "another rank of the job could not reserve memory for the sequence of pricings.");
        }
        K = 1;
        for (int k = 1; k <= 32; ++k)
            if (vote[k] > 0.0) { K = k; break; }
    } else if (err) {
        return fail(err, err_text.c_str());
    }
    *K_out = K < 2 ? 1 : K;
    return 0;
}

static int enqueue_seq_step_multi(omc_ctx* c, const omc_params* p, int n, int K, double* dst)
{
    int rc;
    const int64_t M = p[0].n_paths;
    const int N = p[0].n_steps;
    const int sem = p[0].semantics;
    const int64_t ld = padded_ld(M);
    const size_t sbytes = sizeof(float) * (size_t)ld * (size_t)(N + 1);
    const size_t o_sx = 0, o_tex = o_sx + up256(sizeof(float) * (size_t)M), o_ex = o_tex + up256(sizeof(int32_t) * (size_t)M),
                 o_part = o_ex + up256(sizeof(float) * (size_t)M + 16), o_betas = o_part + up256(sizeof(double) * 2 * 8 * omc::kMaxLsmBlocks),
                 per = o_betas + up256(sizeof(double) * 4 * (size_t)(N + 1));
    const size_t gbytes = up256(sizeof(double) * 8 * (size_t)K * (size_t)(N + 1));
    if ((rc = seq_multi_alloc(c, M, N, K))) return rc;  // (the layout above)
    const size_t eb = omc::lsm_sweep_args_bytes(), tbytes = eb * (size_t)K;
    constexpr int kSlots = 32;
    constexpr size_t kSlotBytes = 32 * 1024;
    if (tbytes > kSlotBytes) return fail(-4, "argument table of the multi-pricing sweep exceeds its upload slot.");
    if (!c->mtab_pin) HIP_TRY(hipHostMalloc((void**)&c->mtab_pin, kSlotBytes * kSlots, hipHostMallocDefault));
    omc::LsmWorkspace w0;
    if ((rc = prepare_lsm(c, M, N, p[0].r, p[0].T, false, false, &w0))) return rc;  // discount table (+ unused singles)
    const bool ext = c->distributed();
    const bool vec4 = omc::state_vec4(M);  // ld is a multiple of 64 and every matrix starts 256-byte aligned
    char* state = (char*)c->mstate.p;
    double* gmomK = (double*)state;
    for (int i0 = 0; i0 < n; i0 += K) {
        const int Kb = n - i0 < K ? n - i0 : K;
        const int G = omc::lsm_multi_groups(M, Kb, c->seq_step_wgs > 0 ? c->seq_step_wgs : c->device_cus);
        if (c->mtab_slot == kSlots) {  // the ring wraps: earlier uploads must have been consumed
            HIP_TRY(hipStreamSynchronize(c->stream));
            c->mtab_slot = 0;
        }
        char* img = c->mtab_pin + kSlotBytes * (size_t)c->mtab_slot++;
        for (int k = 0; k < Kb; ++k) {
            const omc_params& q = p[i0 + k];
            char* st = state + gbytes + per * (size_t)k;
            omc::LsmWorkspace w = w0;
            w.sx = (float*)(st + o_sx); w.tex = (int32_t*)(st + o_tex); w.live = (float*)(st + o_ex);
            w.part = (double*)(st + o_part); w.betas = (double*)(st + o_betas);
            w.gmom = gmomK + 8 * (size_t)k; w.gstride = 8 * Kb;
            w.result = dst + 8 * (size_t)(i0 + k);
            omc::LsmProblem prob{(const float*)((char*)c->mS.p + sbytes * (size_t)k), ld, M, N, q.is_put ? 1 : 0, q.K, q.r, q.T};
            omc::lsm_sweep_args_image(prob, w, sem, false, img + eb * (size_t)k, ext);
        }
        HIP_TRY(hipMemcpyAsync(c->mtable.p, img, eb * (size_t)Kb, hipMemcpyHostToDevice, c->stream));
        const bool p2p = ext && p2p_active(c) && Kb <= omc::kP2PMaxPricings;
        if (p2p) {  // where each pricing's partials are and where its global moments go
            const double* parts[omc::kP2PMaxPricings];
            double* gm[omc::kP2PMaxPricings];
            int nb[omc::kP2PMaxPricings], gs[omc::kP2PMaxPricings];
            for (int k = 0; k < Kb; ++k) {
                parts[k] = (const double*)(state + gbytes + per * (size_t)k + o_part);
                gm[k] = gmomK + 8 * (size_t)k;
                nb[k] = omc::lsm_sweep_blocks(M);
                gs[k] = 8 * Kb;
            }
            HIP_TRY(omc::p2p_set_jobs(c->p2p, c->stream, parts, gm, nb, gs, Kb));
        }
        if (i0 == 0 && p2p) omc::p2p_begin_call(c->p2p);  // its first exchange absorbs start-up skew
        if (i0 == 0) HIP_TRY(hipEventRecord(c->ev[0], c->stream));
        for (int k = 0; k < Kb; ++k)
            if ((rc = enqueue_paths(c, &p[i0 + k], (float*)((char*)c->mS.p + sbytes * (size_t)k), ld))) return rc;
        if (i0 == 0) HIP_TRY(hipEventRecord(c->ev[1], c->stream));
        for (int t = N; t >= 1; --t) {
            HIP_TRY(omc::lsm_step_multi(c->stream, c->mtable.p, Kb, G, sem, vec4, N, t));
            if (ext && t >= 2) {
                if (p2p) {
                    HIP_TRY(omc::p2p_exchange_step_multi(c->p2p, c->stream, Kb, t - 1));
                    c->p2p_used = true;
                } else {
                    HIP_TRY(omc::lsm_reduce_step_moments_multi(c->stream, c->mtable.p, Kb, t - 1));
                    if ((rc = allreduce(c, gmomK + (size_t)(t - 1) * 8 * (size_t)Kb, 8 * Kb))) return rc;  // K fits' moments, one collective
                }
            }
        }
        HIP_TRY(omc::lsm_final_multi(c->stream, c->mtable.p, Kb, M));
        if (i0 == 0) HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    }
    return 0;
}

int omc_seq_step_width(omc_ctx* c, const omc_params* p, int n)
{
    if (!c || !p || n <= 0) return 0;
    for (int i = 0; i < n; ++i)
        if (check_params(&p[i])) return 0;
    return seq_multi_width(c, p, n);
}

// ---- two-pass flow on folded storage: the small launches of K pricings of one geometry shared ----------------
// Per pricing the stream carries six dependent launches, three of them latency-bound: the pass-1 reduction (N - 1
// workgroups), the table build (N + 1 workgroups of two waves that wait on a dependency chain) and the finalize (ONE
// workgroup) -- at 1M paths x 252 steps 36 + 5 + 5 = 46 us of the 362 us of kernel time of a pricing
// (profiles/r08_seq_group_kernel_stats.txt), during which the chip is nearly empty; the kernel boundaries between them
// cost next to nothing beside that.  A run of pricings that agree in geometry and fold constants is therefore priced in groups of K:
//     for k: generator(k) -> S[k]; pass-1 sweep(k) -> part1[k]        (single launches; the generator stays in front
//     ONE launch: the K reductions        part1[k] -> gmom[k]          of ITS pass 1, no pass 2 behind a generator)
//     ONE launch: the K table builds      gmom[k] -> betas[k], crit[k]
//     for k: pass-2 sweep(k) -> part[k]
//     ONE launch: the K finalizes         part[k], gmom[k] -> result slot of the pricing
// The three launches take the pricing from grid.y and run the bodies of the single launches (omc_lsm.hip), so res[i]
// keeps the bits of omc_price_american(p[i]).  One stream, no host wait and no grid-wide barrier inside a group.
// The members' buffers, workspaces, slots and the three launches are TwoPassGroup's (omc_ctx.h; shared with the option chain);
// the sequence's own: a generator per member in front of its pass-1 sweep, the members' events, ONE fold table per run.
// One card only: a distributed context all-reduces every pricing's moment table between its pass 1 and its fits.

// pricing `q` can be a member of a group (the context is not distributed)
static bool seq_group_eligible(const omc_ctx* c, const omc_params* q)
{
    return c->pass2_tables && q->semantics == OMC_SEM_TWO_PASS && q->n_steps >= 2 && fold_applies(c, q);
}

// how many pricings from p[0] on form one run: eligible, same geometry, ONE fold table and ONE discount table
static int seq_group_run(const omc_ctx* c, const omc_params* p, int n)
{
    if (c->distributed() || !seq_group_eligible(c, &p[0])) return 1;
    double c0, g;
    omc::gbm_fold_constants(p[0].S0, p[0].K, p[0].r, p[0].sigma, p[0].T, p[0].n_steps, &c0, &g);
    int run = 1;
    for (; run < n; ++run) {
        const omc_params& q = p[run];
        if (!seq_group_eligible(c, &q) || q.n_paths != p[0].n_paths || q.n_steps != p[0].n_steps || q.r != p[0].r ||
            q.T != p[0].T)
            break;
        double c0q, gq;
        omc::gbm_fold_constants(q.S0, q.K, q.r, q.sigma, q.T, q.n_steps, &c0q, &gq);
        if (c0q != c0 || gq != g) break;
    }
    return run;
}

// bytes of one member's folded path matrix (its small buffers: GroupLayout)
static size_t seq_group_matrix_bytes(const omc_params* p)
{
    return sizeof(float) * (size_t)padded_ld(p->n_paths / 2) * ((size_t)p->n_steps + 1);
}

// The width a run of `run` pricings like p[0] asks for.  Default (profiles/r08_seq_group_sweep.txt): sharing saves a
// fixed ~35 us of small kernels per pricing, and the big kernels of a group run 2-3 % slower than back to back on one
// matrix, a loss that grows with the pricing's own time, i.e. with paths x steps.  Measured at 252 steps, groups of 8
// against single pricings: 1.26 x at 65,536 paths, 1.09 x at 1M, 1.02 x at 2M, 1.00 x at 4M, 0.99 x at 8M (16: under 2 %
// more at any size, for twice the resident path matrices).  So pricings of more than 2^29 path-steps (2.1M paths x 252
// steps) stay single.  (Fewer steps, more paths, all below the bound: 2M x 50 1.12 x, 4M x 126 1.015 x, 8M x 50 1.01 x.)
static int seq_group_ideal(const omc_ctx* c, const omc_params* p, int run)
{
    if (run < 2) return 1;
    static const int env_k = getenv("OMC_SEQ_TWO_PASS_K") ? atoi(getenv("OMC_SEQ_TWO_PASS_K")) : -1;
    int k = c->seq_two_pass_k >= 0 ? c->seq_two_pass_k : env_k;
    if (k < 0) k = (double)p[0].n_paths * (double)p[0].n_steps > 536870912.0 ? 1 : 8;
    if (k > omc::kSeqGroupMax) k = omc::kSeqGroupMax;
    if (k > run) k = run;
    return k < 2 ? 1 : k;
}

// ... and what this card has room for: the byte budget of the per-step flows' resident matrices (seq_multi_fit)
static int seq_group_fit(const omc_ctx* c, const omc_params* p, int k)
{
    const GroupLayout L(p[0].n_paths, p[0].n_steps);
    const int fit = (int)(seq_resident_budget(c, c->gS.cap + c->gstate.cap) / ((double)seq_group_matrix_bytes(p) + (double)L.per));
    if (k > fit) k = fit;
    return k < 2 ? 1 : k;
}

// Reserve the group buffers; no room (a shared card, option "alloc_limit"): halve K down to one pricing at a time
// instead of failing the sequence.
static int seq_group_reserve(omc_ctx* c, const omc_params* p, int run, int* K_out)
{
    *K_out = 1;
    int K = seq_group_ideal(c, p, run);
    const GroupLayout L(p[0].n_paths, p[0].n_steps);
    const size_t sbytes = seq_group_matrix_bytes(p);
    // (buffers that are large enough already need no look at the card's free memory: the query takes a quarter of a
    // millisecond during which the stream runs dry at the head of every sequence)
    if (K >= 2 && (c->gS.cap < sbytes * (size_t)K || c->gstate.cap < L.per * (size_t)K)) K = seq_group_fit(c, p, K);
    // (a buffer that has to grow is freed first, while an earlier, smaller group of the same sequence may still be
    // running in it: hipFree waits for the device before it releases memory, so that group ends undisturbed)
    while (K >= 2) {
        int rc = c->gS.ensure(sbytes * (size_t)K);
        if (!rc) rc = c->gstate.ensure(L.per * (size_t)K);
        if (!rc) break;
        if (rc != (int)hipErrorOutOfMemory && rc != (int)hipErrorMemoryAllocation) return rc;
        K /= 2;
    }
    *K_out = K < 2 ? 1 : K;
    return 0;
}

// pricings p[i0 .. i0 + Kb) as one group; their sums go to dst + 8 i
static int enqueue_seq_group(omc_ctx* c, const omc_params* p, int i0, int Kb, double* dst)
{
    int rc;
    const int64_t M = p[i0].n_paths;
    const int N = p[i0].n_steps;
    const size_t sbytes = seq_group_matrix_bytes(&p[i0]);
    int64_t ld = 0;
    const double* cK = nullptr;
    if ((rc = plan_storage(c, &p[i0], 0, &ld, &cK))) return rc;  // the group's one fold table
    omc::LsmWorkspace w0;
    if ((rc = prepare_lsm(c, M, N, p[i0].r, p[i0].T, true, false, &w0))) return rc;  // discount table (+ the singles)
    if (!cK || ld != padded_ld(M / 2) || Kb > omc::kSeqGroupMax) return fail(-4, "a grouped two-pass sequence needs folded storage.");
    TwoPassGroup grp(GroupLayout(M, N), c->gstate.p, w0, true);
    hipEvent_t* evs[omc::kSeqGroupMax];
    for (int k = 0; k < Kb; ++k) {  // the event pool grows, and may move, HERE: the members' event sets are fetched
        hipEvent_t* grown = nullptr;  // below, once it no longer does
        if ((rc = pricing_events(c, i0 + k, &grown))) return rc;
    }
    for (int k = 0; k < Kb; ++k) {
        const omc_params& q = p[i0 + k];
        float* S = (float*)((char*)c->gS.p + sbytes * (size_t)k);
        omc::LsmProblem prob{S, ld, M, N, q.is_put ? 1 : 0, q.K, q.r, q.T};
        prob.fold_cK = cK;
        grp.add(prob, dst + 8 * (size_t)(i0 + k));
        if ((rc = pricing_events(c, i0 + k, &evs[k]))) return rc;
        if (evs[k]) {  // a timed pricing: events around ITS generator, pass-1 sweep and (below) pass-2 sweep
            grp.w[k].ev_p1_end = evs[k][4]; grp.w[k].ev_p2_end = evs[k][6];
            HIP_TRY(hipEventRecord(evs[k][0], c->stream));
        }
        if ((rc = enqueue_paths(c, &q, S, ld, true))) return rc;
        if (evs[k]) HIP_TRY(hipEventRecord(evs[k][1], c->stream));
        HIP_TRY(omc::lsm_pass1_sweep(c->stream, prob, grp.w[k], &grp.g.ntiles));
    }
    HIP_TRY(grp.reduce_pass1(c->stream));
    HIP_TRY(grp.build_tables(c->stream));
    for (int k = 0; k < Kb; ++k) {
        if (evs[k]) HIP_TRY(hipEventRecord(evs[k][5], c->stream));
        HIP_TRY(omc::lsm_pass2_sweep(c->stream, grp.prob[k], grp.w[k], false, true, &grp.g.nblk));
    }
    HIP_TRY(grp.finalize(c->stream));
    if (i0 == 0) HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    return 0;
}

int omc_seq_group_width(omc_ctx* c, const omc_params* p, int n)
{
    if (!c || !p || n <= 0) return 0;
    for (int i = 0; i < n; ++i)
        if (check_params(&p[i])) return 0;
    const int run = seq_group_run(c, p, n);
    const int k = seq_group_ideal(c, p, run);
    return k < 2 ? 1 : seq_group_fit(c, p, k);
}

// n pricings back to back on the stream with NO host synchronisation in between: pricing i + 1 is
// enqueued while pricing i runs, every pricing's sums land in their own slot of a host-mapped buffer,
// one wait at the end.  Results are those of n omc_price_american calls; kernel times are measured on
// the first pricing, ms_total is the average over the sequence (first launch to last completion).
int omc_price_american_seq(omc_ctx* c, const omc_params* p, int n, omc_result* res)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!p || !res || n <= 0) return fail(-7, "null pointer or empty sequence.");
    for (int i = 0; i < n; ++i)
        if ((rc = check_params(&p[i]))) return rc;
    if (!c->hres_dev) {  // no host-mapped memory on this system: one pricing at a time
        for (int i = 0; i < n; ++i)
            if ((rc = omc_price_american(c, &p[i], &res[i], nullptr, 0))) return rc;
        return 0;
    }
    if (c->seq_cap < n) {
        if (c->seq_pin) (void)hipHostFree(c->seq_pin);
        c->seq_pin = c->seq_dev = nullptr;
        c->seq_cap = 0;
        HIP_TRY(hipHostMalloc((void**)&c->seq_pin, sizeof(double) * 8 * (size_t)n, hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer((void**)&c->seq_dev, c->seq_pin, 0));
        c->seq_cap = n;
    }
    hipEvent_t ev_end = c->ev[2];
    if (!c->ev_seq) HIP_TRY(hipEventCreate(&c->ev_seq));
    ev_end = c->ev_seq;
    const bool overlapped = seq_can_overlap(c, p, n);
    int multi = 1;
    if (!overlapped && (rc = seq_multi_reserve(c, p, n, &multi))) return rc;
    if (overlapped && (rc = enqueue_seq_overlapped(c, p, n, c->seq_pin))) return rc;
    // across GPUs the sums stay in device memory (one slot per pricing) and are all-reduced together after
    // the last pricing -- the hook / communicator sees ONE call with 8n doubles -- then copied out
    const bool dist = c->distributed() && !overlapped;
    if (dist && (rc = c->seq_local.ensure(sizeof(double) * 8 * (size_t)n))) return rc;
    double* local = (double*)c->seq_local.p;
    c->defer_result_allreduce = dist;
    if (multi > 1 && (rc = enqueue_seq_step_multi(c, p, n, multi, dist ? local : c->seq_dev))) {
        c->defer_result_allreduce = false;
        return rc;
    }
    for (int i = 0; i < n && !overlapped && multi <= 1;) {
        // a run of two-pass pricings of one geometry on folded storage: in groups that share their small launches; a
        // single pricing left over, a run that is not to be grouped, and everything else, one at a time
        int run = seq_group_run(c, &p[i], n - i), Kg = 1;
        if (run >= 2 && (rc = seq_group_reserve(c, &p[i], run, &Kg))) break;
        while (Kg >= 2 && run >= 2 && !rc) {
            const int Kb = Kg < run ? Kg : run;
            rc = enqueue_seq_group(c, p, i, Kb, c->seq_dev);
            i += Kb;
            run -= Kb;
        }
        for (; run >= 1 && !rc; ++i, --run) {
            hipEvent_t* evs = nullptr;
            if ((rc = pricing_events(c, i, &evs))) break;
            rc = enqueue_pricing(c, &p[i], nullptr, 0, dist ? local + 8 * (size_t)i : c->seq_dev + 8 * (size_t)i,
                                 evs, nullptr);
            if (!rc && evs && i == 0 && hipEventRecord(evs[2], c->stream) != hipSuccess) rc = fail(999, "hipEventRecord failed");
        }
        if (rc) break;
    }
    c->defer_result_allreduce = false;
    if (rc) return rc;
    if (dist) {
        if (c->p2p_used) HIP_TRY(omc::p2p_stamp_results(c->p2p, c->stream, local, n));  // (enqueue_lsm stamps one at a time)
        if ((rc = allreduce(c, local, 8 * n))) return rc;
        HIP_TRY(hipMemcpyAsync(c->seq_pin, local, sizeof(double) * 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipEventRecord(ev_end, c->stream));
    if ((rc = wait_stream(c))) return rc;
    if ((rc = check_p2p(c, c->seq_pin, n))) return rc;
    float ms_all = 0;
    HIP_TRY(hipEventElapsedTime(&ms_all, c->ev[0], ev_end));
    // kernel times: a pricing that carried events reports its own, the others those of the latest one before them
    omc_result timed;
    memset(&timed, 0, sizeof timed);
    for (int i = 0; i < n; ++i) {
        hipEvent_t* evs = nullptr;  // (the K-per-launch flow times its first launch only)
        if ((multi <= 1 || i == 0) && (rc = pricing_events(c, i, &evs))) return rc;
        if (evs) {
            if ((rc = read_kernel_times(evs, &p[i], &timed, i == 0))) return rc;
            if (multi > 1) timed.ms_paths /= (double)multi;  // ev[0]..ev[1] spans the first batch's K generators
        }
        fill_result(&res[i], c->seq_pin + 8 * (size_t)i, c->distributed() ? p[i].n_paths * c->world : p[i].n_paths,
                    c->distributed() ? c->world : 1);
        res[i].ms_paths = timed.ms_paths;
        res[i].ms_pass1 = timed.ms_pass1;
        res[i].ms_pass2 = timed.ms_pass2;
        res[i].ms_total = ms_all / (float)n;
        res[i].ms_lsm = res[i].ms_total - timed.ms_paths;
        res[i].timed = evs ? 1 : 0;
        res[i].folded = fold_applies(c, &p[i]) ? 1 : 0;
    }
    return 0;
}

}  // extern "C"
