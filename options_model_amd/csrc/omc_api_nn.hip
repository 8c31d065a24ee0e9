// omc_api_nn.hip -- the network entry points (include/omc.h): the per-step ContNet flow, the MLP pass 2 / trainer,
// the local-vol generator, the training rows, the seven-feature OLS and the sharded trainer.
#include <algorithm>

#include "omc_ctx.h"

using namespace omc::abi;

// A failure only this rank can see, in a call that is collective on a context with a communicator / hook: kept rather
// than returned, so that the rank still enters the collectives its peers have entered; the job then fails together.
struct RankFailure {
    int code = 0;
    std::string text;
    void note(int rc) { code = rc; text = g_err; }
    int raise() const { return fail(code, text.c_str()); }
};

// The first all-reduce of a collective fit, with this rank's failure riding along as a flag: v[0..6] = the sum over the
// ranks of n_r mean_r, v[7] = the sum of n_r (st = n_r, mean_r[7], ..; a failed rank adds zeros), v[8] = ranks that
// failed.  -> 0, or the error every rank returns together: its own on a failed rank, peer_code / peer_text elsewhere.
static int allreduce_means(omc_ctx* c, const double* st, const RankFailure& f, int peer_code, const char* peer_text,
                           double v[9])
{
    int rc;
    if ((rc = c->seq_vote.ensure(kVoteBytes))) return rc;  // (never allocates: exists since the communicator / hook was installed)
    const double nr = f.code ? 0.0 : st[0];
    for (int q = 0; q < 7; ++q) v[q] = nr * st[1 + q];
    v[7] = nr;
    v[8] = f.code ? 1.0 : 0.0;
    if ((rc = allreduce_host(c, (double*)c->seq_vote.p, v, 9))) return rc;
    if (v[8] > 0.0) return f.code ? f.raise() : fail(peer_code, peer_text);
    return 0;
}

extern "C" {

// ------------------------------------------------------------------ per-step ContNet flow (v1 / v2 regressor)
namespace {

// The reference's per-step loop (Options_model.py:112-151 = options_model_2.py:283-312) on a device path
// matrix: for t = N-1 .. 1 { set = in the money & not exercised; skip if empty; fresh net; `epochs` full-batch
// Adam steps; exercise where payoff > net(input) }.  One host read per step (the set's size, which sizes the
// trainer's launches); everything else is stream-ordered.  Leaves the valuation sums in w.result.
int contnet_sweep(omc_ctx* c, const omc::LsmProblem& p, omc::LsmWorkspace& w, int hidden, int epochs, double lr,
                  uint64_t seed, double* rows_total)
{
    int rc;
    const int H = omc::cn_padded_width(hidden);
    const int np = omc::mlp_param_count(H, 2);
    const int64_t M = p.M;
    const int N = p.N;
    if ((rc = c->cn_scratch.ensure(omc::cn_scratch_bytes(M)))) return rc;
    if ((rc = c->cn_net.ensure(sizeof(float) * 3 * (size_t)np))) return rc;
    if ((rc = c->cn_cont.ensure(sizeof(float) * (size_t)M))) return rc;
    if ((rc = c->mlp_wt.ensure(omc::mlp_wt_bytes(H, 2)))) return rc;
    if ((rc = c->mlp_loss.ensure(sizeof(double)))) return rc;
    HIP_TRY(hipMemsetAsync(c->mlp_loss.p, 0, sizeof(double), c->stream));  // the trainer adds its losses here (unused)
    float* net = (float*)c->cn_net.p;
    w.cont = (const float*)c->cn_cont.p;
    w.ldc = 0;  // one row, rewritten every step
    const double* hdr_dev = omc::cn_header(p, c->cn_scratch.p);
    *rows_total = 0.0;
    HIP_TRY(omc::lsm_step(c->stream, p, w, OMC_SEM_REFERENCE, N, false));  // state: nobody has exercised
    for (int t = N - 1; t >= 1; --t) {
        const double Dt = c->hD[(size_t)(N - t)];
        HIP_TRY(omc::cn_count(c->stream, p, w, c->cn_scratch.p, t, Dt));
        double hdr[4];
        HIP_TRY(hipMemcpyAsync(hdr, hdr_dev, sizeof hdr, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        const int64_t R = (int64_t)hdr[0];
        if (R <= 0) continue;  // `if not np.any(itm): continue`
        *rows_total += (double)R;
        if ((rc = c->cn_data.ensure(sizeof(float) * 8 * (size_t)R))) return rc;
        if ((rc = c->mlp_part.ensure(omc::mlp_partial_bytes(H, 2, R)))) return rc;
        HIP_TRY(omc::cn_rows(c->stream, p, w, c->cn_scratch.p, t, Dt, (float*)c->cn_data.p));
        HIP_TRY(omc::cn_init(c->stream, hidden, t, seed, net, net + np, net + 2 * (size_t)np));
        omc::MlpTrainPlan plan;
        plan.data = (const float*)c->cn_data.p;
        plan.params = net; plan.adam_m = net + np; plan.adam_v = net + 2 * (size_t)np;
        plan.partial = (float*)c->mlp_part.p; plan.loss_acc = (double*)c->mlp_loss.p;
        plan.nrows = R; plan.batch = R; plan.hidden = H; plan.layers = 2;
        plan.wt = (float*)c->mlp_wt.p;
        plan.lr = lr; plan.beta1 = 0.9; plan.beta2 = 0.999; plan.eps = 1e-8;  // optim.Adam defaults
        plan.weight_decay = 0.0; plan.dropout = 0.0; plan.seed = 0; plan.shuffle_key = 0;
        for (int e = 0; e < epochs; ++e) {
            plan.first_step = e;
            plan.wt_current = e > 0;
            HIP_TRY(omc::mlp_train_steps(c->stream, plan));
        }
        HIP_TRY(omc::cn_forward(c->stream, p, w, c->cn_scratch.p, t, Dt, hidden, net, (float*)c->cn_cont.p));
        HIP_TRY(omc::lsm_step(c->stream, p, w, OMC_SEM_REFERENCE, t, false));
    }
    return 0;
}

int finish_contnet(omc_ctx* c, const omc::LsmProblem& p, omc::LsmWorkspace& w, double rows_total, omc_result* res,
                   float* sx_out, int32_t* tex_out)
{
    int rc;
    HIP_TRY(omc::lsm_final_reduce(c->stream, p, w, 1, true, sx_out || tex_out));
    if ((rc = copy_outputs(c, w, p.M, p.N, nullptr, sx_out, tex_out))) return rc;
    c->hres[4] = rows_total;
    fill_result(res, c->hres, p.M);
    return 0;
}

}  // namespace

int omc_lsm_contnet(omc_ctx* c, const float* S, int64_t ld, int64_t n_paths, int n_steps, double K, double r,
                    double T, int is_put, int nn_hidden, int nn_epochs, double nn_lr, uint64_t nn_seed,
                    omc_result* res, float* sx_out, int32_t* tex_out)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if ((rc = check_lsm_args(S, ld, n_paths, n_steps, K, r, T))) return rc;
    if ((rc = check_contnet(c, nn_hidden, nn_epochs, nn_lr))) return rc;
    if (!res) return fail(-7, "null pointer.");
    omc::LsmWorkspace w;
    if ((rc = prepare_lsm(c, n_paths, n_steps, r, T, false, false, &w))) return rc;
    omc::LsmProblem p{S, ld, n_paths, n_steps, is_put ? 1 : 0, K, r, T};
    double rows = 0.0;
    if ((rc = contnet_sweep(c, p, w, nn_hidden, nn_epochs, nn_lr, nn_seed, &rows))) return rc;
    return finish_contnet(c, p, w, rows, res, sx_out, tex_out);
}

/* the initial parameters of step t's net, in the trainer's padded layout (host float32 [n]) */
int omc_contnet_init_params(omc_ctx* c, int nn_hidden, int t, uint64_t nn_seed, float* params_out, int n)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    const int H = omc::cn_padded_width(nn_hidden);
    if (nn_hidden < 1 || H < 0) return fail(-4, "nn_hidden must be in 1 .. 128.");
    const int np = omc::mlp_param_count(H, 2);
    if (!params_out || n != np) return fail(-7, "params_out must hold the padded net's parameters.");
    if ((rc = c->cn_net.ensure(sizeof(float) * 3 * (size_t)np))) return rc;
    float* net = (float*)c->cn_net.p;
    HIP_TRY(omc::cn_init(c->stream, nn_hidden, t, nn_seed, net, net + np, net + 2 * (size_t)np));
    HIP_TRY(hipMemcpyAsync(params_out, net, sizeof(float) * (size_t)np, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int omc_price_american_contnet(omc_ctx* c, const omc_params* p, int nn_hidden, int nn_epochs, double nn_lr,
                               uint64_t nn_seed, omc_result* res)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if ((rc = check_params(p))) return rc;
    if (p->semantics != OMC_SEM_REFERENCE)
        return fail(-4, "the per-step network is the regressor of the reference flow (semantics 0).");
    if ((rc = check_contnet(c, nn_hidden, nn_epochs, nn_lr))) return rc;
    if (!res) return fail(-7, "null result pointer.");
    const int64_t M = p->n_paths;
    const int N = p->n_steps;
    float* S = nullptr; int64_t ld = 0;
    if ((rc = ensure_paths(c, p, Storage::full_only, &S, &ld))) return rc;
    omc::LsmWorkspace w;
    if ((rc = prepare_lsm(c, M, N, p->r, p->T, false, false, &w))) return rc;
    omc::LsmProblem prob{S, ld, M, N, p->is_put ? 1 : 0, p->K, p->r, p->T};
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    if ((rc = enqueue_paths(c, p, S, ld))) return rc;
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    double rows = 0.0;
    if ((rc = contnet_sweep(c, prob, w, nn_hidden, nn_epochs, nn_lr, nn_seed, &rows))) return rc;
    HIP_TRY(omc::lsm_final_reduce(c->stream, prob, w, 1, true, false));
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    HIP_TRY(hipMemcpyAsync(c->hres, w.result, sizeof(double) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->hres[4] = rows;
    fill_result(res, c->hres, M);
    return read_kernel_times(c->ev, p, res);
}

int omc_mlp_param_count(int hidden, int layers) { return omc::mlp_param_count(hidden, layers); }

int omc_mlp_train_supported(int hidden, int layers, int64_t batch)
{
    return omc::mlp_train_kernel_choice(hidden, layers, batch) != 0;
}

int omc_lsm_apply_mlp(omc_ctx* c, const float* S, int64_t ld, int64_t n_paths, int n_steps, double K,
                      double r, double T, int is_put, int hidden, int layers, const float* params,
                      const double* feat_mean, const double* feat_std, double y_mean, double y_std,
                      double dropout, uint64_t seed, omc_result* res, float* sx_out, int32_t* tex_out)
{
    return omc_lsm_apply_mlp_shard(c, S, ld, n_paths, n_steps, K, r, T, is_put, hidden, layers, params, feat_mean, feat_std,
                                   y_mean, y_std, dropout, seed, res, sx_out, tex_out, 0, n_paths / 2);
}

int omc_lsm_apply_mlp_shard(omc_ctx* c, const float* S, int64_t ld, int64_t n_paths, int n_steps, double K,
                            double r, double T, int is_put, int hidden, int layers, const float* params,
                            const double* feat_mean, const double* feat_std, double y_mean, double y_std,
                            double dropout, uint64_t seed, omc_result* res, float* sx_out, int32_t* tex_out,
                            int64_t col_base0, int64_t col_base1)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if ((rc = check_lsm_args(S, ld, n_paths, n_steps, K, r, T))) return rc;
    if (omc_mlp_param_count(hidden, layers) < 0)
        return fail(-9, "pass 2 supports hidden = 32, 64 or 128 with 2 or 3 hidden layers.");
    if (!params || !feat_mean || !feat_std || !res) return fail(-7, "null pointer.");
    if (!(dropout >= 0.0 && dropout < 1.0)) return fail(-4, "dropout must be in [0, 1).");
    for (int i = 0; i < 7; ++i)
        if (!(feat_std[i] > 0.0)) return fail(-4, "feature standard deviations must be positive.");
    omc::LsmWorkspace w;
    if ((rc = prepare_lsm(c, n_paths, n_steps, r, T, false, true, &w))) return rc;
    omc::LsmProblem p{S, ld, n_paths, n_steps, is_put ? 1 : 0, K, r, T};
    HIP_TRY(omc::mlp_apply_pass2(c->stream, p, hidden, layers, params, feat_mean, feat_std, y_mean, y_std,
                                 dropout, seed, w.sx, w.tex, col_base0, col_base1));
    HIP_TRY(omc::lsm_final_reduce(c->stream, p, w, 1));
    if ((rc = copy_outputs(c, w, n_paths, n_steps, nullptr, sx_out, tex_out))) return rc;
    fill_result(res, c->hres, n_paths);
    return 0;
}

int omc_localvol_param_count(int hidden, int layers) { return omc::localvol_param_count(hidden, layers); }

int omc_localvol_paths_f32(omc_ctx* c, float* S, int64_t ld, int64_t n_paths, int n_steps, double S0,
                           double r, double T, double K, int hidden, int layers, const float* params,
                           double m_scale, double tau_scale, double epsilon, const float* Z)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if ((rc = check_market(S0, K, T, r))) return rc;
    if ((rc = check_sizes(n_paths, n_steps))) return rc;
    if ((rc = check_matrix(S, ld, n_paths))) return rc;
    if (omc_localvol_param_count(hidden, layers) < 0)
        return fail(-9, "the local-vol kernel supports hidden_dim = 64 with 1..8 hidden layers.");
    if (!params || !Z) return fail(-7, "null pointer.");
    if (n_paths & 1) return fail(-3, "antithetic layout needs an even n_paths.");
    if (!(m_scale > 0) || !(tau_scale > 0)) return fail(-4, "scaler values must be positive.");
    HIP_TRY(omc::localvol_paths(c->stream, S, ld, n_paths, n_steps, layers, params, Z, S0, r, T, K, m_scale,
                                tau_scale, epsilon));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int omc_nn_build_rows(omc_ctx* c, const float* S, int64_t ld, int64_t n_paths, int n_steps, double K, double r,
                      double T, int is_put, float* data, int64_t cap_rows, int64_t* n_rows, double* stats16)
{
    int rc;
    const RowsCache had = c ? c->rows_cache : RowsCache{};
    if ((rc = bind_in(c))) return rc;
    if ((rc = check_lsm_args(S, ld, n_paths, n_steps, K, r, T))) return rc;
    if (!n_rows || (data && !stats16)) return fail(-7, "null pointer.");
    const bool full = data != nullptr;
    // The count call (data == NULL) already makes the ONE sweep that counts and forms the statistics; when the call with
    // `data` is the very next call on this context with the same arguments, it starts from those results (counts and
    // offsets are still in the context's scratch) and only writes the rows: S is read twice in all, not three times.
    const bool hit = full && had.valid && had.S == S && had.ld == ld && had.M == n_paths && had.N == n_steps &&
                     had.is_put == (is_put ? 1 : 0) && had.K == K && had.r == r && had.T == T;
    // On a context with a communicator / hook the full call is COLLECTIVE (two small all-reduces below).  A failure that
    // only this rank can see -- no memory for its scratch, a row buffer too small for ITS rows, a HIP error -- must not
    // send it home before the peers have entered them: it is carried as a flag in the first all-reduce instead, and
    // every rank of the job returns an error together.
    const bool dist = full && c->distributed();
    RankFailure lerr;
    omc::LsmWorkspace w;
    if ((rc = prepare_lsm(c, n_paths, n_steps, r, T, false, false, &w)) ||
        (rc = c->scratch.ensure(omc::nn_rows_scratch_bytes(n_paths, n_steps)))) {
        if (!dist) return rc;
        lerr.note(rc);
    }
    omc::LsmProblem p{S, ld, n_paths, n_steps, is_put ? 1 : 0, K, r, T};
    int64_t R = 0;
    double st[16] = {0.0};  // n, mean[7], M2[7] of [x, x^2, x^3, max(x-1,0), s, x*s, y] over this rank's rows
    if (!lerr.code && hit) {
        R = had.R;
        memcpy(st, had.st, sizeof st);
    } else if (!lerr.code) {
        // ONE sweep over S: the counts of every (step, tile) and the statistics
        const int64_t* total_dev = nullptr;
        const double* stats_dev = nullptr;
        hipError_t e = omc::nn_rows_count(c->stream, p, w.D, c->scratch.p, &total_dev, &stats_dev);
        if (e == hipSuccess) e = hipMemcpyAsync(&R, total_dev, sizeof R, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(st, stats_dev, sizeof st, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            g_err = std::string("pass 1 of the NN flow failed: ") + hipGetErrorString(e);
            if (!dist) return (int)e;
            lerr.note((int)e);
            R = 0;
        }
    }
    *n_rows = R;
    if (!full) {  // count only: leave the sweep's results for the call with `data`
        RowsCache& k = c->rows_cache;
        k.valid = true; k.S = S; k.ld = ld; k.M = n_paths; k.N = n_steps; k.is_put = is_put ? 1 : 0; k.K = K; k.r = r; k.T = T;
        k.R = R;
        memcpy(k.st, st, sizeof st);
        return 0;
    }
    if (!lerr.code && cap_rows < R) {
        g_err = "row buffer smaller than the number of in-the-money (step, path) pairs.";
        if (!dist) return -6;
        lerr.note(-6);
    }
    for (int i = 0; i < 16; ++i) stats16[i] = i < 7 ? 0.0 : 1.0;
    stats16[0] = 1.0;  // the constant feature: mean 1, std 0 -> 1
    stats16[14] = 0.0;
    double mean[7], m2[7], Rg = (double)R;
    if (!dist) {
        if (R == 0) return 0;
        for (int q = 0; q < 7; ++q) {
            mean[q] = st[1 + q];
            m2[q] = st[8 + q];
        }
    } else {
        // The statistics are those of ALL ranks' rows (the reference trains one network on the rows of all paths):
        // (1) sum over the ranks of n_r mean_r and n_r -> the global means; (2) sum of M2_r + n_r (mean_r - mean)^2 ->
        // the global sum of squared deviations (Chan's merge, for any number of ranks at once).  A rank without rows
        // contributes zeros; when NO rank has a row every rank returns the defaults together.
        double v[9];
        if ((rc = allreduce_means(c, st, lerr, 3102, "another rank of the job could not build its training rows.", v)))
            return rc;
        const double nr = st[0];
        Rg = v[7];
        if (!(Rg > 0.0)) return 0;
        double dv[8];
        for (int q = 0; q < 7; ++q) {
            mean[q] = v[q] / Rg;
            const double dm = st[1 + q] - mean[q];
            dv[q] = nr > 0.0 ? st[8 + q] + nr * dm * dm : 0.0;
        }
        dv[7] = 0.0;
        if ((rc = allreduce_host(c, (double*)c->seq_vote.p, dv, 8))) return rc;
        for (int q = 0; q < 7; ++q) m2[q] = dv[q];
    }
    // layout: feat_mean[0..6], feat_std[7..13], y_mean [14], y_std [15]; population std, zero std -> 1 (:551-563)
    for (int q = 0; q < 6; ++q) {
        const double sd = std::sqrt(m2[q] / Rg);
        stats16[1 + q] = mean[q];
        stats16[8 + q] = sd > 1e-13 * std::fabs(mean[q]) ? sd : 1.0;
    }
    const double ysd = std::sqrt(m2[6] / Rg);
    stats16[14] = mean[6];
    stats16[15] = ysd > 1e-13 * std::fabs(mean[6]) ? ysd : 1.0;
    if (R > 0) {
        HIP_TRY(omc::nn_rows_write(c->stream, p, w.D, c->scratch.p, stats16, stats16 + 7, stats16[14], stats16[15], data,
                                   cap_rows));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// Solve the normal equations of the live (non-constant) standardised columns: A w = b with A = the correlation matrix of
// the columns, b = their correlations with the target; symmetric Gauss elimination with diagonal pivoting, a column
// whose pivot has vanished (exactly collinear with those before it) gets weight 0 -- any solution of a consistent
// singular system predicts the same values, and that is all pass 2 uses.
static void ols7_solve(const double* st, double n, const double* sd, const bool* live, double* w7)
{
    auto C = [&](int i, int j) { return i <= j ? st[8 + i * 7 - i * (i - 1) / 2 + (j - i)] : st[8 + j * 7 - j * (j - 1) / 2 + (i - j)]; };
    int idx[6], m = 0;
    for (int q = 0; q < 6; ++q)
        if (live[q]) idx[m++] = q;
    double A[6][7];
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < m; ++j) A[i][j] = C(idx[i], idx[j]) / (n * sd[idx[i]] * sd[idx[j]]);
        A[i][m] = C(idx[i], 6) / (n * sd[idx[i]] * sd[6]);
    }
    bool used[6] = {false, false, false, false, false, false};
    int order[6], rank = 0;
    for (int k = 0; k < m; ++k) {
        int pv = -1;
        double best = 1e-13;  // (unit diagonal: a pivot below this is rounding noise of an exactly dependent column)
        for (int i = 0; i < m; ++i)
            if (!used[i] && A[i][i] > best) { best = A[i][i]; pv = i; }
        if (pv < 0) break;
        used[pv] = true;
        order[rank++] = pv;
        for (int i = 0; i < m; ++i) {
            if (i == pv) continue;
            const double f = A[i][pv] / A[pv][pv];
            if (f == 0.0) continue;
            for (int j = 0; j <= m; ++j) A[i][j] -= f * A[pv][j];
        }
    }
    for (int q = 0; q < 7; ++q) w7[q] = 0.0;  // column 0 is the constant: normalised to zero, minimum-norm weight 0
    for (int k = 0; k < rank; ++k) w7[1 + idx[order[k]]] = A[order[k]][m] / A[order[k]][order[k]];
}

// The body of omc_lsm_ols7 / omc_price_american_ols7 behind their argument checks (which are the same on every rank).
// On a context with a communicator / hook the call is COLLECTIVE (two small all-reduces for the fit, one for the result).
// A failure only this rank can see -- no memory for its path matrix or workspace (`lerr`: what the caller already ran
// into), a HIP error in its sweep or in its pass 2 -- travels as a flag: in the ninth double of the first all-reduce
// (allreduce_means), resp. in slot 7 of the result sums (which the kernels leave at zero), and every rank returns an error
// together (the rank's own code there, 3103 on its peers) instead of leaving the peers inside a collective.
static int lsm_ols7_run(omc_ctx* c, const float* S, int64_t ld, int64_t n_paths, int n_steps, double K, double r, double T,
                        int is_put, omc_result* res, double* weights7, double* stats16, float* sx_out, int32_t* tex_out,
                        RankFailure lerr)
{
    int rc;
    const bool dist = c->distributed();
    omc::LsmWorkspace w;
    if (!lerr.code && ((rc = prepare_lsm(c, n_paths, n_steps, r, T, false, true, &w)) ||
                  (rc = c->scratch.ensure(omc::ols7_scratch_bytes(n_paths, n_steps))))) {
        if (!dist) return rc;
        lerr.note(rc);
    }
    if (lerr.code && !dist) return lerr.raise();
    omc::LsmProblem p{S, ld, n_paths, n_steps, is_put ? 1 : 0, K, r, T};
    // pass 1 (:482-516): one sweep -> (n, mean, co-moments) of the 6 non-constant features and the target
    double st[omc::kOls7Stats] = {0.0};
    if (!lerr.code) {
        const double* stats_dev = nullptr;
        hipError_t e = omc::ols7_comoments(c->stream, p, w.D, c->scratch.p, &stats_dev);
        if (e == hipSuccess) e = hipMemcpyAsync(st, stats_dev, sizeof st, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            g_err = std::string("the co-moment sweep failed: ") + hipGetErrorString(e);
            if (!dist) return (int)e;
            lerr.note((int)e);
        }
    }
    if (dist) {
        // The fit is over ALL ranks' rows (paths shard by antithetic pair, the regression does not): the ranks' triples
        // (n_r, mean_r, C_r) are merged by Chan's formula for any number of ranks at once -- (1) sum of n_r mean_r and
        // n_r -> the global means; (2) sum of C_r + n_r (mean_r - mean)(mean_r - mean)^T -> the global co-moments -- the
        // "regression moments" all-reduce of north_star, 9 + 28 doubles.  Every rank then solves the same 6 x 6 system.
        double v[9];
        if ((rc = allreduce_means(c, st, lerr, 3103, "another rank of the job could not run its co-moment sweep.", v)))
            return rc;
        const double nr = st[0], ng = v[7];
        double cg[28];
        for (int i = 0, k = 0; i < 7; ++i)
            for (int j = i; j < 7; ++j, ++k) {
                const double di = ng > 0.0 ? st[1 + i] - v[i] / ng : 0.0, dj = ng > 0.0 ? st[1 + j] - v[j] / ng : 0.0;
                cg[k] = nr > 0.0 ? st[8 + k] + nr * di * dj : 0.0;
            }
        if ((rc = allreduce_host(c, (double*)c->seq_vote.p, cg, 28))) return rc;
        st[0] = ng;
        for (int q = 0; q < 7; ++q) st[1 + q] = ng > 0.0 ? v[q] / ng : 0.0;
        for (int k = 0; k < 28; ++k) st[8 + k] = cg[k];
    }
    const double n = st[0];
    // normalisation (:550-563): population std, zero std -> 1 (the column is then all zero)
    double s16[16], sd[7], w7[7];
    bool live[7];
    for (int i = 0; i < 16; ++i) s16[i] = i < 7 ? 0.0 : 1.0;
    s16[0] = 1.0;
    s16[14] = 0.0;
    for (int q = 0; q < 7; ++q) w7[q] = 0.0;
    if (n > 0.0) {
        // The sweep's quantities are g = [u, u^2, u^3, max(u, 0), s, u s, y] with u = x - 1 (what the per-step polynomial uses):
        // the same span as the reference's features f = [x, x^2, x^3, max(x - 1, 0), s, x s] plus the constant -- the same
        // fit -- but a far better conditioned Gram matrix for in-the-money spots, which sit within a few tens of percent
        // of the strike (the normal equations carry eps * cond^2).  f = B g + b with a unit lower-triangular B:
        //   x = u + 1, x^2 = u^2 + 2 u + 1, x^3 = u^3 + 3 u^2 + 3 u + 1, x s = u s + s.
        // The system is solved for g; means, stds and weights are then stated for f, the reference's features.
        static const double B[6][6] = {{1, 0, 0, 0, 0, 0}, {2, 1, 0, 0, 0, 0}, {3, 3, 1, 0, 0, 0},
                                       {0, 0, 0, 1, 0, 0}, {0, 0, 0, 0, 1, 0}, {0, 0, 0, 0, 1, 1}};
        static const double b0[6] = {1, 1, 1, 0, 0, 0};
        auto Cg = [&](int i, int j) { return i <= j ? st[8 + i * 7 - i * (i - 1) / 2 + (j - i)] : st[8 + j * 7 - j * (j - 1) / 2 + (i - j)]; };
        double sdg[7];
        bool liveg[7];
        for (int q = 0; q < 7; ++q) {
            const double mean = st[1 + q], v = std::sqrt(Cg(q, q) / n);
            // (u is centred near 0: its own size is no yardstick for "constant" -- the spot's is, x = u + 1)
            const double scale = q < 3 ? 1.0 : std::fabs(mean);
            liveg[q] = v > 1e-13 * scale;
            sdg[q] = liveg[q] ? v : 1.0;
        }
        double wg[7];
        for (int q = 0; q < 7; ++q) wg[q] = 0.0;
        if (liveg[6]) ols7_solve(st, n, sdg, liveg, wg);  // (a constant target: every weight 0, continuation = its mean)
        // the reference's features: means, population stds (zero -> 1, :562), and the weights c = B^-T a, a = wg / sdg
        double a[6], cf[6];
        for (int q = 0; q < 6; ++q) a[q] = wg[1 + q] / sdg[q];
        cf[5] = a[5];
        cf[4] = a[4] - cf[5];
        cf[3] = a[3];
        cf[2] = a[2];
        cf[1] = a[1] - 3.0 * cf[2];
        cf[0] = a[0] - 2.0 * cf[1] - 3.0 * cf[2];
        for (int i = 0; i < 6; ++i) {
            double mean = b0[i], var = 0.0;
            for (int j = 0; j < 6; ++j) {
                mean += B[i][j] * st[1 + j];
                for (int k = 0; k < 6; ++k) var += B[i][j] * B[i][k] * Cg(j, k);
            }
            const double v = std::sqrt(std::fmax(var, 0.0) / n);
            live[i] = v > 1e-13 * std::fabs(mean);
            sd[i] = live[i] ? v : 1.0;
            s16[1 + i] = mean;
            s16[8 + i] = sd[i];
            w7[1 + i] = live[i] ? cf[i] * sd[i] : 0.0;  // (a constant column contributes (f - mean) = 0 whatever its weight)
        }
        live[6] = liveg[6];
        sd[6] = sdg[6];
        s16[14] = st[7];
        s16[15] = sd[6];
    }
    // pass 2 (:615-651) with the fit, then the mean of the cash-flows valued at t = dt (:651)
    hipError_t e2 = omc::ols7_pass2(c->stream, p, s16, s16 + 7, w7, s16[14], s16[15], w.sx, w.tex);
    if (e2 == hipSuccess) e2 = omc::lsm_final_reduce(c->stream, p, w, 1);
    if (e2 != hipSuccess) {
        g_err = std::string("pass 2 with the fit failed: ") + hipGetErrorString(e2);
        if (!dist) return (int)e2;
        lerr.note((int)e2);
        static const double kOne = 1.0;  // this rank's flag rides in slot 7 of the sums about to be all-reduced
        (void)hipMemcpyAsync(w.result + 7, &kOne, sizeof kOne, hipMemcpyHostToDevice, c->stream);
    }
    if (dist && (rc = allreduce(c, w.result, 8))) return rc;  // the discounted-payoff sums of all ranks (+ the flag)
    if ((rc = copy_outputs(c, w, n_paths, n_steps, nullptr, lerr.code ? nullptr : sx_out, lerr.code ? nullptr : tex_out)))
        return rc;
    if (dist && (lerr.code || c->hres[7] > 0.0))
        return lerr.code ? lerr.raise() : fail(3103, "another rank of the job could not run its pass 2.");
    fill_result(res, c->hres, c->distributed() ? n_paths * c->world : n_paths, c->distributed() ? c->world : 1);
    res->sum_nitm = (int64_t)llround(n);  // rows of the regression (of the job)
    if (weights7) memcpy(weights7, w7, sizeof w7);
    if (stats16) memcpy(stats16, s16, sizeof s16);
    return 0;
}

int omc_lsm_ols7(omc_ctx* c, const float* S, int64_t ld, int64_t n_paths, int n_steps, double K, double r, double T,
                 int is_put, omc_result* res, double* weights7, double* stats16, float* sx_out, int32_t* tex_out)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if ((rc = check_lsm_args(S, ld, n_paths, n_steps, K, r, T))) return rc;
    if (!res) return fail(-7, "null result pointer.");
    return lsm_ols7_run(c, S, ld, n_paths, n_steps, K, r, T, is_put, res, weights7, stats16, sx_out, tex_out, RankFailure());
}

int omc_price_american_ols7(omc_ctx* c, const omc_params* p, omc_result* res, double* weights7, double* stats16)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if ((rc = check_params(p))) return rc;
    if (!res) return fail(-7, "null result pointer.");
    // the context's own path matrix: the largest allocation of the call and the likeliest to fail on a card shared with
    // other tenants -- on a distributed context that failure must reach the peers (lsm_ols7_run), not strand them
    float* S = nullptr; int64_t ld = 0;
    RankFailure pre;
    if ((rc = ensure_paths(c, p, Storage::full_only, &S, &ld)) || (rc = enqueue_paths(c, p, S, ld))) {
        if (!c->distributed()) return rc;
        pre.note(rc);
    }
    return lsm_ols7_run(c, S, ld, p->n_paths, p->n_steps, p->K, p->r, p->T, p->is_put ? 1 : 0, res, weights7, stats16,
                        nullptr, nullptr, pre);
}

int omc_nn_feature_stats(omc_ctx* c, const double* x, const int32_t* t, const double* y, int64_t n_rows,
                         double T, double dt, double* out16)
{
    int rc = bind_in(c);
    if (rc) return rc;
    if (!x || !t || !y || !out16) return fail(-7, "null pointer.");
    if (n_rows <= 0) return fail(-3, "n_rows must be positive.");
    if ((rc = c->scratch.ensure(omc::nn_stats_scratch_bytes() + sizeof(double) * 16))) return rc;
    double* scratch = (double*)c->scratch.p;
    double* dev16 = scratch + omc::nn_stats_scratch_bytes() / sizeof(double);
    HIP_TRY(omc::nn_feature_stats(c->stream, x, t, y, n_rows, T, dt, scratch, dev16));
    HIP_TRY(hipMemcpyAsync(out16, dev16, sizeof(double) * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int omc_mlp_train_variant(int hidden, int layers, int64_t batch)
{
    return omc::mlp_train_kernel_choice(hidden, layers, batch);
}

int omc_mlp_dropout_masks(omc_ctx* c, int variant, int hidden, int layers, int64_t n_rows, const uint32_t* keys,
                          uint32_t step, uint64_t seed, double dropout, uint8_t* out)
{
    int rc = bind_in(c);
    if (rc) return rc;
    if (variant < 0 || variant > 4) return fail(-4, "variant must be 0 (pass 2) or 1 .. 4 (omc_mlp_train_variant).");
    const bool shape_ok = (variant == 3 || variant == 0) ? (hidden == 32 || hidden == 64 || hidden == 128)
                        : variant == 1 ? hidden == 64 : (hidden == 64 || hidden == 128);
    if (!shape_ok || layers < 1 || layers > 3) return fail(-9, "this kernel does not exist for that network shape.");
    if (n_rows <= 0 || !out) return fail(-3, "n_rows must be positive, out non-null.");
    if (!(dropout >= 0.0 && dropout < 1.0)) return fail(-4, "dropout must be in [0, 1).");
    const size_t nout = (size_t)layers * (size_t)n_rows * (size_t)hidden, nkey = keys ? sizeof(uint32_t) * (size_t)n_rows : 0;
    if ((rc = c->scratch.ensure(nout + nkey + 16))) return rc;
    uint8_t* dout = (uint8_t*)c->scratch.p;
    uint32_t* dkeys = keys ? (uint32_t*)(dout + ((nout + 15) & ~(size_t)15)) : nullptr;
    if (keys) HIP_TRY(hipMemcpyAsync(dkeys, keys, nkey, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(omc::mlp_dropout_masks(c->stream, variant, hidden, layers, n_rows, dkeys, step, seed, dropout, dout));
    HIP_TRY(hipMemcpyAsync(out, dout, nout, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int omc_mlp_shuffle_indices(omc_ctx* c, int64_t n_rows, uint64_t shuffle_key, int64_t* out_device)
{
    int rc = bind_in(c);
    if (rc) return rc;
    if (n_rows <= 0 || !out_device) return fail(-3, "n_rows must be positive, out non-null.");
    HIP_TRY(omc::mlp_shuffle_indices(c->stream, n_rows, shuffle_key, out_device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int omc_mlp_train_epoch(omc_ctx* c, const float* data, int64_t n_rows, int64_t batch, int hidden,
                        int layers, float* params, float* adam_m, float* adam_v, int64_t* step,
                        double lr, double beta1, double beta2, double eps, double weight_decay,
                        double dropout, uint64_t seed, uint64_t shuffle_key, double* mean_loss)
{
    int rc = bind_in(c);
    if (rc) return rc;
    if (omc::mlp_train_kernel_choice(hidden, layers, batch) == 0)
        return fail(-9, "the fused trainer supports hidden = 32, 64 or 128 with 2 or 3 hidden layers.");
    if (!data || !params || !adam_m || !adam_v || !step || !mean_loss) return fail(-7, "null pointer.");
    if (n_rows <= 0 || batch <= 0 || *step < 0) return fail(-3, "n_rows, batch must be positive.");
    if (!(dropout >= 0.0 && dropout < 1.0)) return fail(-4, "dropout must be in [0, 1).");
    if (!(lr > 0.0)) return fail(-4, "learning rate must be positive.");
    if ((rc = c->mlp_part.ensure(omc::mlp_partial_bytes(hidden, layers, batch)))) return rc;
    if ((rc = c->mlp_wt.ensure(omc::mlp_wt_bytes(hidden, layers)))) return rc;
    if ((rc = c->mlp_loss.ensure(sizeof(double)))) return rc;
    HIP_TRY(hipMemsetAsync(c->mlp_loss.p, 0, sizeof(double), c->stream));
    omc::MlpTrainPlan t;
    t.data = data; t.params = params; t.adam_m = adam_m; t.adam_v = adam_v;
    t.partial = (float*)c->mlp_part.p; t.loss_acc = (double*)c->mlp_loss.p;
    t.nrows = n_rows; t.batch = batch; t.first_step = *step; t.hidden = hidden; t.layers = layers;
    t.wt = (float*)c->mlp_wt.p;
    t.lr = lr; t.beta1 = beta1; t.beta2 = beta2; t.eps = eps; t.weight_decay = weight_decay;
    t.dropout = dropout; t.seed = seed; t.shuffle_key = shuffle_key;
    t.allow_q16 = true;
    const int64_t nb = (n_rows + batch - 1) / batch;
    HIP_TRY(omc::mlp_train_steps(c->stream, t));
    double acc = 0.0;
    HIP_TRY(hipMemcpyAsync(&acc, c->mlp_loss.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *step += nb;
    *mean_loss = acc / (double)nb;
    return 0;
}

// ---- the NN regressor sharded over the ranks of a job (options_model_3.py:542-613)
int omc_nn_half_counts(omc_ctx* c, const float* S, int64_t ld, int64_t n_paths, int n_steps, double K, int is_put,
                       int64_t* counts)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if ((rc = check_sizes(n_paths, n_steps))) return rc;
    if ((rc = check_matrix(S, ld, n_paths))) return rc;
    if (!counts) return fail(-7, "null pointer.");
    if (n_steps < 2) return 0;
    const size_t bytes = sizeof(int64_t) * 2 * (size_t)(n_steps - 1);
    if ((rc = c->scratch.ensure(bytes))) return rc;
    omc::LsmProblem p{S, ld, n_paths, n_steps, is_put ? 1 : 0, K, 0.0, 1.0};
    HIP_TRY(omc::nn_rows_half_counts(c->stream, p, n_paths / 2, (int64_t*)c->scratch.p));
    HIP_TRY(hipMemcpyAsync(counts, c->scratch.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int omc_mlp_shard_epoch(omc_ctx* c, const float* data, int64_t n_rows_local, int64_t rows_global, int64_t batch,
                        uint64_t shuffle_key, const int64_t* gstart, const int64_t* lstart, int nseg, int segs_per_step,
                        float* data_epoch, uint32_t* drop_pos, int64_t* step_off)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if (!gstart || !lstart || !step_off || (n_rows_local > 0 && (!data || !data_epoch || !drop_pos)))
        return fail(-7, "null pointer.");
    if (n_rows_local < 0 || rows_global <= 0 || batch <= 0 || nseg <= 0 || n_rows_local > rows_global)
        return fail(-3, "row counts, batch and segment count must be positive.");
    if (gstart[0] != 0 || gstart[nseg] != rows_global) return fail(-4, "segment table does not cover [0, rows_global).");
    const int64_t steps = (rows_global + batch - 1) / batch;
    // scratch: segment tables | selection scan | sel_row, sel_i | step offsets
    const size_t tab = sizeof(int64_t) * (size_t)(2 * nseg + 1), scan = omc::mlp_shard_scratch_bytes(rows_global),
                 sel = sizeof(int64_t) * (size_t)(n_rows_local + 1), so = sizeof(int64_t) * (size_t)(steps + 1);
    if ((rc = c->shard.ensure(up256(tab) + up256(scan) + 2 * up256(sel) + up256(so)))) return rc;
    char* b = (char*)c->shard.p;
    int64_t* d_g = (int64_t*)b;
    int64_t* d_l = d_g + nseg + 1;
    void* d_scan = b + up256(tab);
    int64_t* sel_row = (int64_t*)(b + up256(tab) + up256(scan));
    int64_t* sel_i = (int64_t*)((char*)sel_row + up256(sel));
    int64_t* d_so = (int64_t*)((char*)sel_i + up256(sel));
    HIP_TRY(hipMemcpyAsync(d_g, gstart, sizeof(int64_t) * (size_t)(nseg + 1), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_l, lstart, sizeof(int64_t) * (size_t)nseg, hipMemcpyHostToDevice, c->stream));
    // own segments must tile [0, n_rows_local) of the rank's matrix: checked here, on the host, before any kernel
    // indexes `data` with them
    {
        std::vector<std::pair<int64_t, int64_t>> own;
        for (int s = 0; s < nseg; ++s) {
            if (gstart[s + 1] < gstart[s]) return fail(-4, "segment table is not ascending.");
            if (lstart[s] >= 0 && gstart[s + 1] > gstart[s]) own.push_back({lstart[s], gstart[s + 1] - gstart[s]});
        }
        std::sort(own.begin(), own.end());
        int64_t at = 0;
        for (auto& o : own) {
            if (o.first != at) return fail(-4, "this rank's segments do not tile its rows.");
            at += o.second;
        }
        if (at != n_rows_local) return fail(-4, "this rank's segments do not add up to its row count.");
    }
    const int64_t* total_dev = nullptr;
    const int group = (segs_per_step > 0 && nseg % segs_per_step == 0) ? segs_per_step : 0;
    HIP_TRY(omc::mlp_shard_select(c->stream, rows_global, shuffle_key, d_g, d_l, nseg, group, d_scan, sel_row, sel_i, &total_dev));
    HIP_TRY(omc::mlp_shard_gather(c->stream, data, sel_row, sel_i, n_rows_local, batch, steps, data_epoch, drop_pos, d_so));
    int64_t total = -1;
    HIP_TRY(hipMemcpyAsync(&total, total_dev, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(step_off, d_so, sizeof(int64_t) * (size_t)(steps + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (total != n_rows_local) return fail(-4, "the epoch's permutation selected another number of rows than the rank owns.");
    return 0;
}

static int allreduce_cb(void* user, double* dptr, int count) { return allreduce((omc_ctx*)user, dptr, count); }

int omc_mlp_train_epoch_sharded(omc_ctx* c, const float* data_epoch, int64_t n_rows_local, int64_t rows_global,
                                int64_t batch, int hidden, int layers, float* params, float* adam_m, float* adam_v,
                                int64_t* step, double lr, double beta1, double beta2, double eps, double weight_decay,
                                double dropout, uint64_t seed, const int64_t* step_off, const uint32_t* drop_pos,
                                double* mean_loss)
{
    int rc = bind_in(c);
    if (rc) return rc;
    if (!params || !adam_m || !adam_v || !step || !mean_loss || !step_off || (n_rows_local > 0 && (!data_epoch || !drop_pos)))
        return fail(-7, "null pointer.");
    if (n_rows_local < 0 || rows_global <= 0 || batch <= 0 || *step < 0) return fail(-3, "row counts, batch must be positive.");
    if (!(dropout >= 0.0 && dropout < 1.0)) return fail(-4, "dropout must be in [0, 1).");
    if (!(lr > 0.0)) return fail(-4, "learning rate must be positive.");
    const int64_t steps = (rows_global + batch - 1) / batch;
    if (step_off[0] != 0 || step_off[steps] != n_rows_local) return fail(-4, "step offsets do not cover the rank's rows.");
    for (int64_t k = 0; k < steps; ++k)
        if (step_off[k + 1] < step_off[k] || step_off[k + 1] - step_off[k] > batch) return fail(-4, "step offsets are not ascending.");
    omc::MlpTrainPlan t;
    t.data = data_epoch; t.params = params; t.adam_m = adam_m; t.adam_v = adam_v;
    t.nrows = n_rows_local; t.batch = batch; t.first_step = *step; t.hidden = hidden; t.layers = layers;
    t.lr = lr; t.beta1 = beta1; t.beta2 = beta2; t.eps = eps; t.weight_decay = weight_decay;
    t.dropout = dropout; t.seed = seed; t.shuffle_key = 0;
    t.allow_q16 = true;
    t.step_off = step_off; t.rows_global = rows_global; t.drop_pos = drop_pos;
    t.allreduce = allreduce_cb; t.allreduce_user = c;  // no communicator / hook: the sum of one rank
    const int64_t kb = omc::mlp_plan_kernel_batch(t);
    if (omc::mlp_train_kernel_choice(hidden, layers, kb) == 0)
        return fail(-9, "the fused trainer supports hidden = 32, 64 or 128 with 2 or 3 hidden layers.");
    const int np = omc::mlp_param_count(hidden, layers);
    if ((rc = c->mlp_part.ensure(omc::mlp_partial_bytes(hidden, layers, kb)))) return rc;
    if ((rc = c->mlp_wt.ensure(omc::mlp_wt_bytes(hidden, layers)))) return rc;
    if ((rc = c->mlp_loss.ensure(sizeof(double)))) return rc;
    if ((rc = c->mlp_gred.ensure((sizeof(double) + sizeof(float)) * (size_t)(np + 1)))) return rc;
    HIP_TRY(hipMemsetAsync(c->mlp_loss.p, 0, sizeof(double), c->stream));
    t.partial = (float*)c->mlp_part.p; t.loss_acc = (double*)c->mlp_loss.p; t.wt = (float*)c->mlp_wt.p;
    t.gred = (double*)c->mlp_gred.p;
    HIP_TRY(omc::mlp_train_steps(c->stream, t));
    double acc = 0.0;
    HIP_TRY(hipMemcpyAsync(&acc, c->mlp_loss.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *step += steps;
    *mean_loss = acc / (double)steps;
    return 0;
}

int omc_mlp_train_batch_supported(int hidden, int layers, int64_t batch)
{
    return omc::mlp_batch_supported(hidden, layers, batch) ? 1 : 0;
}

int omc_mlp_train_epoch_batch(omc_ctx* c, omc_mlp_job* jobs, int n, int hidden, int layers, double beta1, double beta2,
                              double eps, double weight_decay, double dropout)
{
    int rc = bind_in(c);
    if (rc) return rc;
    if (!jobs || n <= 0) return fail(-7, "empty batch.");
    if (n > 65535) return fail(-3, "batch too large (max 65535 networks per call).");
    if (!(dropout >= 0.0 && dropout < 1.0)) return fail(-4, "dropout must be in [0, 1).");
    int64_t max_steps = 0, max_batch32 = 0, max_batch16 = 0, last_step = 0;
    size_t part_bytes = 0;
    const int64_t q16_rows = omc::mlp_q16_rows(hidden);
    for (int i = 0; i < n; ++i) {
        const omc_mlp_job& j = jobs[i];
        if (!j.data || !j.params || !j.adam_m || !j.adam_v) return fail(-7, "null pointer.");
        if (j.n_rows <= 0 || j.batch <= 0 || j.step < 0) return fail(-3, "n_rows, batch must be positive.");
        if (!(j.lr > 0.0)) return fail(-4, "learning rate must be positive.");
        if (!omc::mlp_batch_supported(hidden, layers, j.batch))
            return fail(-9, "the batched trainer covers the one-tile-per-workgroup shapes (64 | 128 units x 2 | 3 layers at "
                            "minibatches of at most 8192 rows, 32 units x 2 | 3 layers).");
        const int64_t nb = (j.n_rows + j.batch - 1) / j.batch;
        if (nb > max_steps) max_steps = nb;
        // every network runs the kernel its own omc_mlp_train_epoch call runs (16-row tiles up to q16_rows rows)
        if (j.batch <= q16_rows) max_batch16 = std::max<int64_t>(max_batch16, j.batch);
        else max_batch32 = std::max<int64_t>(max_batch32, j.batch);
        part_bytes = std::max(part_bytes, omc::mlp_partial_bytes(hidden, layers, j.batch));
        if (j.step + nb > last_step) last_step = j.step + nb;
    }
    if (max_steps > 0x7fffffff) return fail(-3, "too many steps per epoch.");
    const size_t pb = up256(part_bytes), wb = up256(omc::mlp_wt_bytes(hidden, layers) + 16);
    const size_t lb = up256(sizeof(double) * (size_t)n);
    if ((rc = c->mb_slab.ensure(lb + (pb + wb) * (size_t)n))) return rc;
    if ((rc = c->mb_table.ensure(omc::mlp_batch_table_bytes(n)))) return rc;
    // 1 - beta^step for every step this epoch can reach
    const size_t need = (size_t)last_step + 2;
    if ((rc = adam_bias_tables(c, beta1, beta2, need, need * 2 + 1024))) return rc;
    char* slab = (char*)c->mb_slab.p;
    double* loss = (double*)slab;
    std::vector<omc::MlpBatchJob> hj((size_t)n);
    for (int i = 0; i < n; ++i) {
        omc::MlpBatchJob& b = hj[(size_t)i];
        b.data = jobs[i].data; b.nrows = jobs[i].n_rows; b.batch = jobs[i].batch; b.first_step = jobs[i].step;
        b.params = jobs[i].params; b.adam_m = jobs[i].adam_m; b.adam_v = jobs[i].adam_v;
        b.partial = (float*)(slab + lb + (pb + wb) * (size_t)i);
        b.wt = (float*)(slab + lb + (pb + wb) * (size_t)i + pb);
        b.loss_acc = loss + i;
        b.lr = jobs[i].lr; b.seed = jobs[i].seed; b.shuffle_key = jobs[i].shuffle_key;
        b.allow_q16 = true;
    }
    c->h_table.resize(omc::mlp_batch_table_bytes(n));
    omc::mlp_batch_table_image(hj.data(), n, hidden, layers, beta1, beta2, eps, weight_decay, dropout, c->h_table.data());
    HIP_TRY(hipMemcpyAsync(c->mb_table.p, c->h_table.data(), c->h_table.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(loss, 0, sizeof(double) * (size_t)n, c->stream));
    HIP_TRY(omc::mlp_train_epoch_batch(c->stream, c->mb_table.p, n, hidden, layers, max_steps, (int)((max_batch32 + 31) / 32),
                                       (int)((max_batch16 + 15) / 16),
                                       (const double*)c->mb_bc.p, (const double*)c->mb_bc.p + c->mb_bc_cap));
    c->h_bres.resize((size_t)n);
    HIP_TRY(hipMemcpyAsync(c->h_bres.data(), loss, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; ++i) {
        const int64_t nb = (jobs[i].n_rows + jobs[i].batch - 1) / jobs[i].batch;
        jobs[i].step += nb;
        jobs[i].mean_loss = c->h_bres[(size_t)i] / (double)nb;
    }
    return 0;
}

}  // extern "C"
