// omc_api_chain_greeks.hip -- omc_price_american_chain_greeks (include/omc_chain_greeks.h): the frozen-policy pathwise
// Greeks of every strike, side and exercise schedule of one expiry from ONE generator launch and ONE path matrix
// (DESIGN.md section 35).
//     fold tables, schedule tables, the entries' slots (one upload) -> generator -> S
//     per group of up to 16 entries:
//         pass-1 sweeps -> part1[j]          the chain's own: one per entry, on the matrix or the entry's view
//         ONE launch: the reductions         part1[j] -> gmom[j]       (+ the gather of omc_chain.h where pass 1 walked all rows)
//         ONE launch: the solves             gmom[j] -> betas[j]
//         the Greeks sweeps -> part[j]       one launch per side and "chain_greeks_k" entries
//         ONE launch: the finalizes          part[j], gmom[j] -> the entry's 24 sums
// With the caller's policies (`betas`) pass 1, the reductions and the solves fall away.  One stream, one host wait at the end.
// Pass 1 is omc_price_american_chain's, launch for launch; the solve, the sweep and the finalize run the bodies of
// omc_price_american_greeks' kernels in their geometry: an American entry carries the bits of its single call.
#include <algorithm>

#include "../../include/omc_chain_greeks.h"
#include "omc_chain_greeks.h"
#include "omc_ctx.h"

using namespace omc::abi;

extern "C" int omc_price_american_chain_greeks(omc_ctx* c, const omc_params* p, const omc_chain_entry* e, int n, double bump,
                                               const double* betas, double* betas_out, omc_greeks* out,
                                               omc_chain_greeks_info* info)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!e) return fail(-7, "null entries.");
    if ((rc = check_chain(c, p, e, n))) return rc;
    if (!(bump > 0.0 && bump <= 0.5)) return fail(-4, "bump must lie in (0, 0.5].");
    if (!out) return fail(-7, "null result pointer.");
    const int64_t M = p->n_paths;
    const int N = p->n_steps;
    const size_t n1 = (size_t)N + 1;
    omc_params q0 = *p;
    q0.K = e[0].K;
    q0.is_put = e[0].is_put;
    const bool folded = fold_applies(c, &q0);  // (depends on neither the strike nor the side)
    const int64_t ld = folded ? padded_ld(M / 2) : padded_ld(M);
    if ((rc = c->S.ensure(sizeof(float) * (size_t)ld * n1))) return rc;
    float* S = (float*)c->S.p;
    // the schedules, as omc_price_american_chain cuts them: k in 2 .. N, 0 where every date is one
    omc::ChainSchedules sch;
    memset(&sch, 0, sizeof sch);
    bool bermudan = false;
    for (int i = 0; i < n; ++i) {
        const int k = std::min(e[i].exercise_every, N);
        sch.every[i] = k >= 2 ? k : 0;
        bermudan = bermudan || k >= 2;
    }
    const bool given = betas != nullptr;
    const int G = std::min(n, omc::kChainGroupMax);
    const int ngroups = (n + G - 1) / G;
    const int width = c->chain_greeks_k > 0 ? std::min(c->chain_greeks_k, omc::kChainGreeksMax) : omc::kChainGreeksMax;
    const GroupLayout L(M, N);
    if ((rc = c->gstate.ensure(L.per * (size_t)G))) return rc;
    omc::LsmWorkspace w0;
    memset(&w0, 0, sizeof w0);
    w0.gstride = 8;
    w0.part1_tiles = (int64_t)omc::lsm_part1_tiles(M);
    if ((rc = ensure_discounts(c, N, p->r, p->T, &w0.D))) return rc;
    // the sweep's geometry: the MATRIX's, for every entry (a view's alignment must not choose the column width)
    omc::ChainGreeksArgs ga;
    memset(&ga, 0, sizeof ga);
    {
        omc::GreeksArgs m;
        memset(&m, 0, sizeof m);
        m.S = S; m.ld = ld; m.cols = folded ? M / 2 : M;
        ga.cols = m.cols; ga.vec = omc::greeks_vec(m); ga.nblk = omc::greeks_blocks(m);
    }
    ga.Nf = N; ga.gbm = p->model == OMC_MODEL_GBM ? 1 : 0; ga.order = c->chain_greeks_order;
    ga.S0 = p->S0; ga.r = p->r; ga.sigma = p->sigma; ga.T = p->T; ga.h = bump;
    const size_t part_per = sizeof(double) * omc::kGreeksQ * (size_t)ga.nblk;
    if ((rc = c->cg_part.ensure(part_per * (size_t)G))) return rc;
    if ((rc = c->cg_res.ensure(sizeof(double) * omc::kGreeksQ * (size_t)n))) return rc;
    if ((rc = c->cg_slots.ensure(sizeof(omc::ChainGreeksSlot) * (size_t)n))) return rc;
    double* dres = (double*)c->cg_res.p;
    ga.slots = (const omc::ChainGreeksSlot*)c->cg_slots.p;
    while (c->ev_pool.size() < 2 * (size_t)ngroups) {
        hipEvent_t ev = nullptr;
        HIP_TRY(hipEventCreate(&ev));
        c->ev_pool.push_back(ev);
    }
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    // the entries' fold tables and the Bermudan entries' tables on their scheduled dates: the chain's, launch for launch
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
    // group gi's members, as omc_price_american_chain adds them: a Bermudan entry is the view of its scheduled rows
    auto fill_group = [&](TwoPassGroup& grp, int gi) {
        const int i0 = gi * G, Kb = std::min(G, n - i0);
        for (int k = 0; k < Kb; ++k) {
            const int i = i0 + k;
            omc::LsmProblem q{S, ld, M, N, e[i].is_put, e[i].K, p->r, p->T};
            q.fold_cK = folded ? fold + fstride * (size_t)i : nullptr;
            if (const int every = sch.every[i]) {
                const int Nv = omc::chain_view_steps(N, every);
                q.S = S + (int64_t)(N - every * Nv) * ld;
                q.ld = ld * every;
                q.N = Nv;
                if (folded) q.fold_cK = sched + fstride * (3 * (size_t)i + 2);
            }
            grp.add(q, nullptr);
        }
    };
    // the group's slots hold its puts first, then its calls: order[gi G + s] = the member in slot s
    std::vector<int> order((size_t)n);
    c->cg_hslots.resize(sizeof(omc::ChainGreeksSlot) * (size_t)n);  // (pageable: the context keeps it until the wait below)
    omc::ChainGreeksSlot* hslots = (omc::ChainGreeksSlot*)c->cg_hslots.data();
    for (int gi = 0; gi < ngroups; ++gi) {
        const int i0 = gi * G, Kb = std::min(G, n - i0);
        TwoPassGroup grp(L, c->gstate.p, w0, false);
        fill_group(grp, gi);
        int s = i0;
        for (int side = 1; side >= 0; --side)
            for (int k = 0; k < Kb; ++k)
                if (e[i0 + k].is_put == side) order[(size_t)s++] = k;
        for (s = i0; s < i0 + Kb; ++s) {
            const int k = order[(size_t)s], i = i0 + k;
            omc::ChainGreeksSlot& sl = hslots[(size_t)s];
            sl.S = grp.prob[k].S; sl.ld = grp.prob[k].ld;
            sl.betas = grp.w[k].betas;
            sl.gmom = given ? nullptr : grp.w[k].gmom;
            sl.cK = grp.prob[k].fold_cK;
            sl.D = sch.every[i] ? sched + fstride * (3 * (size_t)i + 1) : w0.D;
            sl.part = (double*)((char*)c->cg_part.p + part_per * (size_t)k);
            sl.result = dres + omc::kGreeksQ * (size_t)i;
            sl.K = e[i].K;
            sl.N = grp.prob[k].N;
            sl.every = sch.every[i] ? sch.every[i] : 1;
        }
    }
    HIP_TRY(hipMemcpyAsync(c->cg_slots.p, hslots, sizeof(omc::ChainGreeksSlot) * (size_t)n, hipMemcpyHostToDevice,
                           c->stream));
    // the caller's policies, restated on the views' rows (view row j is date N - every (Nv - j)); rows 0 and Nv are never read
    std::vector<double>& hgiven = c->cg_hgiven;  // (as the slots: kept by the context)
    if (given) {
        hgiven.assign(4 * n1 * (size_t)n, 0.0);
        for (int i = 0; i < n; ++i) {
            const int every = sch.every[i] ? sch.every[i] : 1;
            const int Nv = sch.every[i] ? omc::chain_view_steps(N, every) : N;
            for (int j = 1; j < Nv; ++j)
                memcpy(&hgiven[4 * (n1 * (size_t)i + (size_t)j)], betas + 4 * (n1 * (size_t)i + (size_t)(N - every * (Nv - j))),
                       sizeof(double) * 4);
        }
    }
    HIP_TRY(hipEventRecord(c->ev[3], c->stream));
    if ((rc = enqueue_paths(c, &q0, S, ld, folded))) return rc;
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    int launches = 0;
    std::vector<double>& hview = c->cg_hview;  // the fits on the views' rows, n1 x 4 doubles per entry (kept by the context)
    if (betas_out && !given) hview.resize(4 * n1 * (size_t)n);
    for (int gi = 0; gi < ngroups; ++gi) {
        const int i0 = gi * G, Kb = std::min(G, n - i0);
        TwoPassGroup grp(L, c->gstate.p, w0, false);
        fill_group(grp, gi);
        const omc::LsmProblem* prob = grp.prob; const omc::LsmWorkspace* w = grp.w;
        omc::ChainGreeksArgs a = ga;
        a.slots = ga.slots + i0;
        int n_fit = 0;  // the longest member's steps
        for (int k = 0; k < Kb; ++k) n_fit = std::max(n_fit, prob[k].N);
        if (given) {
            for (int k = 0; k < Kb; ++k)
                HIP_TRY(hipMemcpyAsync(w[k].betas, &hgiven[4 * n1 * (size_t)(i0 + k)], sizeof(double) * 4 * (size_t)(prob[k].N + 1),
                                       hipMemcpyHostToDevice, c->stream));
        } else {
            // ---- pass 1, as omc_price_american_chain's unfused route runs it (omc_api_chain.hip)
            omc::ChainGatherArgs gt;
            memset(&gt, 0, sizeof gt);
            gt.N = N;
            bool gather = false;
            for (int k = 0; k < Kb; ++k) {
                // rows 0 and N of the fits are only ever copied out
                if (betas_out) HIP_TRY(hipMemsetAsync(w[k].betas, 0, sizeof(double) * 4 * n1, c->stream));
                const int every = sch.every[i0 + k];
                if (every && !folded && prob[k].N >= 2 && omc::rows_aligned(4, M, S, ld)) {
                    gt.gmom[k] = w[k].gmom;
                    gt.every[k] = every;
                    gather = true;
                }
            }
            for (int k = 0; k < Kb; ++k) {
                int64_t nt = 0;
                if (gt.every[k]) {  // full storage with 16-byte loads: all rows, the scheduled ones gathered below
                    omc::LsmProblem all = prob[k];
                    all.S = S; all.ld = ld; all.N = N;
                    HIP_TRY(omc::lsm_pass1_sweep(c->stream, all, w[k], &nt));
                    grp.g.slot[k].N = N;
                    grp.g.N = N;
                } else {
                    omc::LsmWorkspace wk = w[k];
                    if (sch.every[i0 + k]) wk.D = sched + fstride * 3 * (size_t)(i0 + k);  // d1
                    HIP_TRY(omc::lsm_pass1_sweep(c->stream, prob[k], wk, &nt));
                }
                if (nt) grp.g.ntiles = nt;
            }
            HIP_TRY(grp.reduce_pass1(c->stream));
            if (gather) HIP_TRY(omc::chain_gather_moments(c->stream, gt, Kb));
        }
        HIP_TRY(hipEventRecord(c->ev_pool[2 * (size_t)gi], c->stream));
        // ---- the fits, the Greeks sweeps, the sums
        if (!given) HIP_TRY(omc::chain_greeks_solve(c->stream, a, Kb, n_fit));
        int at = 0;
        for (int side = 1; side >= 0; --side) {
            int left = 0;
            for (int k = 0; k < Kb; ++k) left += e[i0 + k].is_put == side ? 1 : 0;
            while (left > 0) {
                const int take = std::min(width, left);
                int n_max = 1;
                for (int s = at; s < at + take; ++s) n_max = std::max(n_max, prob[order[(size_t)(i0 + s)]].N);
                HIP_TRY(omc::chain_greeks_sweep(c->stream, a, at, take, side, folded, n_max));
                ++launches;
                at += take;
                left -= take;
            }
        }
        HIP_TRY(omc::chain_greeks_finalize(c->stream, a, Kb));
        HIP_TRY(hipEventRecord(c->ev_pool[2 * (size_t)gi + 1], c->stream));
        if (betas_out && !given)
            for (int k = 0; k < Kb; ++k) {
                double* to = sch.every[i0 + k] ? hview.data() : betas_out;
                HIP_TRY(hipMemcpyAsync(to + 4 * n1 * (size_t)(i0 + k), w[k].betas, sizeof(double) * 4 * n1, hipMemcpyDeviceToHost,
                                       c->stream));
            }
    }
    std::vector<double>& h = c->cg_hres;  // (a target of the copy below: kept by the context until the wait)
    h.resize(omc::kGreeksQ * (size_t)n);
    HIP_TRY(hipMemcpyAsync(h.data(), dres, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
    if ((rc = wait_stream(c))) return rc;
    // the policy used: an American entry's table as it is; a Bermudan entry's rows at its scheduled dates, zero elsewhere
    for (int i = 0; betas_out && i < n; ++i) {
        const int every = sch.every[i];
        double* to = betas_out + 4 * n1 * (size_t)i;
        if (!every) {
            if (given) memcpy(to, betas + 4 * n1 * (size_t)i, sizeof(double) * 4 * n1);
            continue;
        }
        const int Nv = omc::chain_view_steps(N, every);
        const double* in = (given ? hgiven.data() : hview.data()) + 4 * n1 * (size_t)i;
        memset(to, 0, sizeof(double) * 4 * n1);
        for (int j = 1; j < Nv; ++j) memcpy(to + 4 * (size_t)(N - every * (Nv - j)), in + 4 * (size_t)j, sizeof(double) * 4);
    }
    omc_chain_greeks_info inf;
    memset(&inf, 0, sizeof inf);
    inf.folded = folded ? 1 : 0;
    inf.n_groups = ngroups;
    inf.n_sweep_launches = launches;
    inf.entries_per_launch = width;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[3], c->ev[1]));
    inf.ms_paths = ms;
    hipEvent_t prev = c->ev[1];
    for (int gi = 0; gi < ngroups; ++gi) {
        HIP_TRY(hipEventElapsedTime(&ms, prev, c->ev_pool[2 * (size_t)gi]));
        inf.ms_pass1 += ms;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_pool[2 * (size_t)gi], c->ev_pool[2 * (size_t)gi + 1]));
        inf.ms_greeks += ms;
        prev = c->ev_pool[2 * (size_t)gi + 1];
    }
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], prev));
    inf.ms_total = ms;
    const double Md = (double)M;
    for (int i = 0; i < n; ++i) {
        const double* hi = h.data() + omc::kGreeksQ * (size_t)i;
        omc_greeks* o = &out[i];
        memset(o, 0, sizeof *o);
        fill_result(&o->base, hi, M);
        o->base.folded = inf.folded;
        mean_and_se(hi[8], hi[9], Md, &o->delta, &o->se_delta);
        mean_and_se(hi[10], hi[11], Md, &o->gamma, &o->se_gamma);
        if (ga.gbm) {
            mean_and_se(hi[12], hi[13], Md, &o->vega, &o->se_vega);
            mean_and_se(hi[14], hi[15], Md, &o->rho, &o->se_rho);
            mean_and_se(hi[16], hi[17], Md, &o->theta, &o->se_theta);
        } else {  // no map from the stored spot to the variance path's parameters
            o->vega = o->rho = o->theta = NAN;
            o->se_vega = o->se_rho = o->se_theta = NAN;
        }
        o->bump = bump;
        o->price_up = hi[5] / Md;
        o->price_down = hi[6] / Md;
        o->n_exercised_up = (int64_t)llround(hi[18]);
        o->n_exercised_down = (int64_t)llround(hi[19]);
        o->base.ms_paths = inf.ms_paths;
        o->base.ms_pass1 = inf.ms_pass1;
        o->base.ms_total = inf.ms_total;
        o->base.ms_lsm = inf.ms_total - inf.ms_paths;
        o->base.timed = i == 0 ? 1 : 0;
        o->ms_greeks = inf.ms_greeks;
    }
    if (info) *info = inf;
    return 0;
}
