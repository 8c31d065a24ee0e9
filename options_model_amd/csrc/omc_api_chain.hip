// omc_api_chain.hip -- omc_price_american_chain and omc_chain_width (include/omc.h): many strikes and sides of one expiry
// from ONE generator launch and ONE path matrix.
//     generator -> S;  folded storage: the entries' fold tables cK_j (one launch)
//     per group of up to 16 entries:
//         pass-1 sweeps -> part1[j]      fused: one launch per side and omc_chain_width entries; else one per entry
//         ONE launch: the reductions     part1[j] -> gmom[j]
//         ONE launch: the table builds   gmom[j] -> betas[j], crit[j]        (folded storage with "pass2_tables")
//         pass-2 sweeps -> part[j]       fused / per entry, as above
//         ONE launch: the finalizes      part[j], gmom[j] -> result slot of the entry
// A Bermudan entry (exercise_every >= 2) is the same flow on the view of S that holds its scheduled rows (omc_chain.h,
// DESIGN.md section 24): one more launch in front of the generator gathers its tables, its sweeps are the single
// pricing's on that view, its slot of the shared launches carries the view's length.  A chain that holds one runs unfused.
// A group is a TwoPassGroup (omc_ctx.h), as in the grouped sequences: it carves the entries' buffers from the context's
// group state and issues the three shared launches, every slot carrying its entry's own fold table.
// The unfused sweeps ARE the single pricing's launches (lsm_pass1_sweep, lsm_pass2_sweep), the three shared launches run the
// bodies of its small kernels, and the fused sweeps (omc_chain.hip) form every entry's sums in the single kernels' geometry:
// res[i] carries the bits of omc_price_american(p with e[i]) on every route.  One stream, no host wait before the end.
#include <algorithm>

#include "omc_chain.h"
#include "omc_ctx.h"

using namespace omc::abi;

namespace {

int pow2_floor(int x)
{
    int w = 1;
    while (2 * w <= x) w *= 2;
    return w;
}

// p with the strike and side of one entry: the pricing omc_price_american would be handed
omc_params with_entry(const omc_params* p, const omc_chain_entry& e)
{
    omc_params q = *p;
    q.K = e.K;
    q.is_put = e.is_put;
    return q;
}

}  // namespace

// the checks of the chain's own arguments; `e` may be null when only p and n are to be judged (omc_chain_width).  Shared
// with omc_price_american_chain_greeks (omc_ctx.h).
int omc::abi::check_chain(const omc_ctx* c, const omc_params* p, const omc_chain_entry* e, int n)
{
    int rc;
    if (!p) return fail(-7, "null params.");
    if (n < 1 || n > OMC_CHAIN_MAX) return fail(-3, "a chain has 1 .. 256 entries.");
    omc_params q = *p;  // (p->K and p->is_put are ignored)
    q.K = e ? e[0].K : 1.0;
    if (!(std::isfinite(q.K) && q.K > 0.0)) return fail(-4, "an entry's strike must be finite and positive.");
    if ((rc = check_params(&q))) return rc;
    if (p->semantics != OMC_SEM_TWO_PASS) return fail(-4, "a chain is priced by the two-pass flow (semantics 2).");
    if (!p->antithetic) return fail(-15, "chain paths are antithetic pairs (antithetic = 1).");
    for (int i = 0; e && i < n; ++i) {
        if (!(std::isfinite(e[i].K) && e[i].K > 0.0)) return fail(-4, "an entry's strike must be finite and positive.");
        if (e[i].is_put != 0 && e[i].is_put != 1) return fail(-4, "an entry's is_put must be 0 or 1.");
    }
    for (int i = 0; e && i < n; ++i)
        if (e[i].exercise_every < 0) return fail(-37, "an entry's exercise_every must not be negative (0 or 1: every date).");
    if (c->distributed()) return fail(-10, "a chain is priced on one GPU.");
    return 0;
}

namespace {

// entries per fused launch (0: the unfused route) for the chain's problem on the context's own matrix
int fused_width(const omc_ctx* c, const omc_params* p, int64_t ld, bool folded)
{
    if (!folded || !c->chain_fused || !c->pass2_tables || p->n_steps < 2) return 0;
    omc::LsmProblem prob{(const float*)c->S.p, ld, p->n_paths, p->n_steps, 1, 1.0, p->r, p->T};
    static const double dummy = 0.0;
    prob.fold_cK = &dummy;  // (only says "folded")
    int w = omc::chain_fused_width(prob);
    if (w > 0 && c->chain_k > 0) w = std::min(w, pow2_floor(c->chain_k));
    return w;
}

}  // namespace

extern "C" {

int omc_chain_width(omc_ctx* c, const omc_params* p, int n)
{
    if (!c || check_chain(c, p, nullptr, n)) return 0;
    omc_params q = *p;
    q.K = 1.0;
    const bool folded = fold_applies(c, &q);
    const int w = fused_width(c, p, padded_ld(p->n_paths / 2), folded);
    return w < 1 ? 1 : std::min(w, pow2_floor(n));
}

int omc_price_american_chain(omc_ctx* c, const omc_params* p, const omc_chain_entry* e, int n, omc_result* res,
                             double* betas_out, omc_chain_info* info)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!e || !res) return fail(-7, "null entries or results.");
    if ((rc = check_chain(c, p, e, n))) return rc;
    const int64_t M = p->n_paths;
    const int N = p->n_steps;
    const size_t n1 = (size_t)N + 1;
    const omc_params q0 = with_entry(p, e[0]);
    const bool folded = fold_applies(c, &q0);  // (depends on neither the strike nor the side)
    const int64_t ld = folded ? padded_ld(M / 2) : padded_ld(M);
    if ((rc = c->S.ensure(sizeof(float) * (size_t)ld * n1))) return rc;
    float* S = (float*)c->S.p;
    // the schedules: k cut to 2 .. N (k >= N leaves no early date, as k = N does), 0 where every date is one
    static_assert(omc::kChainMax == OMC_CHAIN_MAX, "ChainSchedules holds one word per entry");
    omc::ChainSchedules sch;
    memset(&sch, 0, sizeof sch);
    bool bermudan = false;
    for (int i = 0; i < n; ++i) {
        const int k = std::min(e[i].exercise_every, N);
        sch.every[i] = k >= 2 ? k : 0;
        bermudan = bermudan || k >= 2;
    }
    const int width = bermudan ? 0 : fused_width(c, p, ld, folded);
    const bool fused = width > 0;
    const bool tables = folded && c->pass2_tables;  // lsm_pass2_tables of every entry
    const int G = std::min(n, omc::kChainGroupMax);
    const GroupLayout L(M, N);
    if ((rc = c->gstate.ensure(L.per * (size_t)G))) return rc;
    if ((rc = c->seq_local.ensure(sizeof(double) * 8 * (size_t)n))) return rc;
    double* dres = (double*)c->seq_local.p;
    // (none of the single pricing's workspace: every entry's buffers are in the group state, no per-path state is written)
    omc::LsmWorkspace w0;
    memset(&w0, 0, sizeof w0);
    w0.gstride = 8;
    w0.crit_irr_every = c->pass2_irr_every;
    w0.part1_tiles = (int64_t)omc::lsm_part1_tiles(M);
    if ((rc = ensure_discounts(c, N, p->r, p->T, &w0.D))) return rc;
    const int ngroups = (n + G - 1) / G;
    while (c->ev_pool.size() < 2 * (size_t)ngroups) {
        hipEvent_t ev = nullptr;
        HIP_TRY(hipEventCreate(&ev));
        c->ev_pool.push_back(ev);
    }
    // ms_total starts HERE: the fold tables are rebuilt by every call and are part of its cost; ms_paths is the generator alone
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    // the entries' fold tables: c0_j from the host (gbm_fold_constants, as plan_storage), the N products on the device
    const size_t fstride = (n1 + 31) / 32 * 32;
    double* fold = nullptr;
    if (folded) {
        if ((rc = c->chain_fold.ensure(sizeof(double) * (fstride + 1) * (size_t)n))) return rc;
        fold = (double*)c->chain_fold.p;
        double* c0_dev = fold + fstride * (size_t)n;
        c->h_table.resize(sizeof(double) * (size_t)n);  // (pageable: the context keeps it until the wait below)
        double* c0 = (double*)c->h_table.data();
        double g = 1.0;
        for (int i = 0; i < n; ++i) omc::gbm_fold_constants(p->S0, e[i].K, p->r, p->sigma, p->T, N, &c0[i], &g);
        HIP_TRY(hipMemcpyAsync(c0_dev, c0, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(omc::chain_fold_tables(c->stream, fold, fstride, c0_dev, n, N, g));
    }
    double* sched = nullptr;  // entry i: [d1 | d2 | cv] at sched + 3 fstride i
    if (bermudan) {
        if ((rc = c->chain_sched.ensure(sizeof(double) * 3 * fstride * (size_t)n))) return rc;
        sched = (double*)c->chain_sched.p;
        HIP_TRY(omc::chain_schedule_tables(c->stream, sched, fstride, w0.D, fold, fstride, sch, n, N));
    }
    HIP_TRY(hipEventRecord(c->ev[3], c->stream));
    if ((rc = enqueue_paths(c, &q0, S, ld, folded))) return rc;
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    int launches = 0;
    std::vector<double> hview;  // the fits of the Bermudan entries on their views' rows, n1 x 4 doubles each
    if (betas_out && bermudan) hview.resize(4 * n1 * (size_t)n);
    for (int gi = 0; gi < ngroups; ++gi) {
        const int i0 = gi * G, Kb = std::min(G, n - i0);
        TwoPassGroup grp(L, c->gstate.p, w0, c->pass2_tables != 0);
        const omc::LsmProblem* prob = grp.prob; const omc::LsmWorkspace* w = grp.w;  // the members, as add() leaves them
        for (int k = 0; k < Kb; ++k) {
            const omc_chain_entry& ek = e[i0 + k];
            omc::LsmProblem q{S, ld, M, N, ek.is_put, ek.K, p->r, p->T};
            q.fold_cK = folded ? fold + fstride * (size_t)(i0 + k) : nullptr;
            if (const int every = sch.every[i0 + k]) {  // the view of the scheduled rows; its row 0 is never read
                const int Nv = omc::chain_view_steps(N, every);
                q.S = S + (int64_t)(N - every * Nv) * ld;
                q.ld = ld * every;
                q.N = Nv;
                if (folded) q.fold_cK = sched + fstride * (3 * (size_t)(i0 + k) + 2);
            }
            grp.add(q, dres + 8 * (size_t)(i0 + k));
            // rows 0 and N of the fits are only ever copied out (prepare_lsm's clear_tables)
            if (betas_out) HIP_TRY(hipMemsetAsync(w[k].betas, 0, sizeof(double) * 4 * n1, c->stream));
        }
        // the fused launches of this group: entries of one side, in pieces of 4 / 2 / 1 up to the width
        struct Piece { int side, first, count; };
        std::vector<Piece> pieces;
        std::vector<int> order;  // the group's entries, puts first
        if (fused) {
            for (int side = 1; side >= 0; --side) {
                const int first = (int)order.size();
                for (int k = 0; k < Kb; ++k)
                    if (e[i0 + k].is_put == side) order.push_back(k);
                for (int at = first, left = (int)order.size() - first; left > 0;) {
                    const int take = std::min(width, pow2_floor(left));
                    pieces.push_back({side, at, take});
                    at += take;
                    left -= take;
                }
            }
        }
        auto sweep_args = [&](const Piece& pc) {
            omc::ChainSweepArgs a;
            memset(&a, 0, sizeof a);
            a.S = S; a.ld = ld; a.P = M / 2; a.N = N; a.KE = pc.count; a.is_put = pc.side; a.D = w0.D;
            for (int j = 0; j < pc.count; ++j) {
                const int k = order[(size_t)(pc.first + j)];
                a.K[j] = prob[k].K; a.invK[j] = 1.0 / prob[k].K; a.cK[j] = prob[k].fold_cK;
                a.part1[j] = w[k].part1; a.crit[j] = w[k].crit; a.betas[j] = w[k].betas; a.part[j] = w[k].part;
            }
            return a;
        };
        // the sweeps of member k: a Bermudan entry's read its own discounts (d1 in pass 1, d2 in pass 2)
        auto swept = [&](int k, int pass) {
            omc::LsmWorkspace wk = w[k];
            if (sch.every[i0 + k]) wk.D = sched + fstride * (3 * (size_t)(i0 + k) + (size_t)pass - 1);
            return wk;
        };
        // pass 1 on full storage with 16-byte loads walks all rows for a Bermudan entry too (omc_chain.h: its row slots
        // do not round alike); the scheduled rows of its moments are gathered after the reduction
        omc::ChainGatherArgs ga;
        memset(&ga, 0, sizeof ga);
        ga.N = N;
        bool gather = false;
        for (int k = 0; k < Kb; ++k) {
            const int every = sch.every[i0 + k];
            if (every && !folded && prob[k].N >= 2 && omc::rows_aligned(4, M, S, ld)) {
                ga.gmom[k] = w[k].gmom;
                ga.every[k] = every;
                gather = true;
            }
        }
        // ---- pass 1
        if (fused) {
            for (const Piece& pc : pieces)
                HIP_TRY(omc::chain_pass1_sweep(c->stream, sweep_args(pc), prob[0], &grp.g.ntiles));
        } else {
            for (int k = 0; k < Kb; ++k) {  // (tiles depend on the columns alone; a view of one row has no pass 1: 0)
                int64_t nt = 0;
                if (ga.every[k]) {
                    omc::LsmProblem all = prob[k];
                    all.S = S; all.ld = ld; all.N = N;
                    HIP_TRY(omc::lsm_pass1_sweep(c->stream, all, w[k], &nt));
                    grp.g.slot[k].N = N;  // (for the reduction: all rows of this member, hence of the grid)
                    grp.g.N = N;
                } else {
                    HIP_TRY(omc::lsm_pass1_sweep(c->stream, prob[k], swept(k, 1), &nt));
                }
                if (nt) grp.g.ntiles = nt;
            }
        }
        HIP_TRY(grp.reduce_pass1(c->stream));
        if (gather) {
            HIP_TRY(omc::chain_gather_moments(c->stream, ga, Kb));
            for (int k = 0; k < Kb; ++k)
                if (ga.every[k]) grp.g.slot[k].N = prob[k].N;
        }
        HIP_TRY(hipEventRecord(c->ev_pool[2 * (size_t)gi], c->stream));
        // ---- pass 2
        if (tables) HIP_TRY(grp.build_tables(c->stream));
        if (fused) {
            for (const Piece& pc : pieces)
                HIP_TRY(omc::chain_pass2_sweep(c->stream, sweep_args(pc), prob[0], &grp.g.nblk));
        } else {
            for (int k = 0; k < Kb; ++k)
                HIP_TRY(omc::lsm_pass2_sweep(c->stream, prob[k], swept(k, 2), false, true, &grp.g.nblk));
        }
        HIP_TRY(grp.finalize(c->stream));
        HIP_TRY(hipEventRecord(c->ev_pool[2 * (size_t)gi + 1], c->stream));
        launches += fused ? (int)pieces.size() : Kb;
        if (betas_out)
            for (int k = 0; k < Kb; ++k) {
                double* to = sch.every[i0 + k] ? hview.data() : betas_out;
                HIP_TRY(hipMemcpyAsync(to + 4 * n1 * (size_t)(i0 + k), w[k].betas, sizeof(double) * 4 * n1,
                                       hipMemcpyDeviceToHost, c->stream));
            }
    }
    std::vector<double> h(8 * (size_t)n);
    HIP_TRY(hipMemcpyAsync(h.data(), dres, sizeof(double) * 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if ((rc = wait_stream(c))) return rc;
    // a Bermudan entry's fits from its view's rows to the dates they belong to; every other row is zero
    for (int i = 0; betas_out && i < n; ++i) {
        const int every = sch.every[i];
        if (!every) continue;
        const int Nv = omc::chain_view_steps(N, every);
        double* out = betas_out + 4 * n1 * (size_t)i;
        const double* in = hview.data() + 4 * n1 * (size_t)i;
        memset(out, 0, sizeof(double) * 4 * n1);
        for (int j = 1; j < Nv; ++j) memcpy(out + 4 * (size_t)(N - every * (Nv - j)), in + 4 * (size_t)j, sizeof(double) * 4);
    }
    omc_chain_info inf;
    memset(&inf, 0, sizeof inf);
    inf.folded = folded ? 1 : 0;
    inf.fused = fused ? 1 : 0;
    inf.n_launch_groups = launches;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[3], c->ev[1]));
    inf.ms_paths = ms;
    hipEvent_t prev = c->ev[1];
    for (int gi = 0; gi < ngroups; ++gi) {
        HIP_TRY(hipEventElapsedTime(&ms, prev, c->ev_pool[2 * (size_t)gi]));
        inf.ms_pass1 += ms;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_pool[2 * (size_t)gi], c->ev_pool[2 * (size_t)gi + 1]));
        inf.ms_pass2 += ms;
        prev = c->ev_pool[2 * (size_t)gi + 1];
    }
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], prev));
    inf.ms_total = ms;
    for (int i = 0; i < n; ++i) {
        fill_result(&res[i], h.data() + 8 * (size_t)i, M);
        res[i].folded = inf.folded;
        res[i].ms_paths = inf.ms_paths;
        res[i].ms_pass1 = inf.ms_pass1;
        res[i].ms_pass2 = inf.ms_pass2;
        res[i].ms_total = inf.ms_total;
        res[i].ms_lsm = inf.ms_total - inf.ms_paths;
        res[i].timed = i == 0 ? 1 : 0;
    }
    if (info) *info = inf;
    return 0;
}

}  // extern "C"
