// omc_api_jump_greeks.hip -- frozen-policy Greeks of American options under jump-diffusion
// (include/omc_jump_greeks.h).  omc_price_american_jump's checks, generator and pass 1 give the
// policy -- or the caller does -- then ONE sweep (omc_jump_greeks.hip) regenerates the paths, prices the base,
// S0 (1 + h) and S0 (1 - h) scenarios with the frozen fits and forms every Greek term.  It replaces pass 2: counts are
// those of omc_price_american_jump and the price differs only in the order of its float64 sum.
#include "../../include/omc_jump_greeks.h"
#include "omc_ctx.h"
#include "omc_jump_greeks.h"

using namespace omc::abi;

extern "C" int omc_price_american_jump_greeks(omc_ctx* c, const omc_params* p, const omc_jump* j, double q, double bump,
                                              const double* betas, double* betas_out, omc_jump_greeks* out)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!out) return fail(-7, "null result pointer.");
    JumpTable t;
    if ((rc = compose_jump(p, j, q, &t, true, false))) return rc;  // the pricing's own checks, codes and table
    if (!(bump > 0.0 && bump <= 0.5)) return fail(-4, "bump must lie in (0, 0.5].");
    if (c->distributed()) return fail(-10, "the jump Greeks sweep runs on one GPU.");
    const int N = p->n_steps;
    const int64_t M = p->n_paths;

    float* S = nullptr;
    int64_t ld = 0;
    if (!betas && (rc = take_full_matrix(c, p, nullptr, &S, &ld))) return rc;  // the caller's fits need no matrix
    omc::LsmWorkspace w;
    if ((rc = prepare_lsm(c, M, N, p->r, p->T, betas == nullptr, betas_out != nullptr, &w))) return rc;
    if (betas && (rc = upload_fits(c, w, betas, N))) return rc;

    // (lambda = 0: every threshold is 2^24, no count word passes one, and the generator writes the vanilla matrix at
    // rate r - q)
    const omc::JumpGen gen{path_spec(c, p, t.drift_rate, S, ld), jump_law(t, j)};
    omc::JumpGreeksArgs g{};
    g.paths = gen.paths;
    g.law = gen.law;
    g.is_put = p->is_put ? 1 : 0;
    g.K = p->K; g.r = p->r; g.h = bump;
    g.lambda = j->lambda; g.sigma_j = j->sigma_j; g.kappa = t.kappa;
    g.D = w.D; g.betas = w.betas; g.gmom = betas ? nullptr : w.gmom;
    const int64_t nwg = omc::jump_greeks_blocks(M);
    if ((rc = c->gk_part.ensure(sizeof(double) * omc::kJumpGreeksQ * (size_t)nwg))) return rc;
    if ((rc = c->gk_res.ensure(sizeof(double) * omc::kJumpGreeksQ))) return rc;
    g.part = (double*)c->gk_part.p;
    g.result = (double*)c->gk_res.p;

    omc::LsmProblem prob{S, ld, M, N, g.is_put, p->K, p->r, p->T};
    w.ev_p1_end = c->ev[4];
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    if (!betas) HIP_TRY(omc::launch_jump_paths(c->stream, gen));
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    const bool fit = betas == nullptr && N >= 2;
    if (fit) {
        HIP_TRY(omc::lsm_pass1_moments(c->stream, prob, w));
        HIP_TRY(omc::lsm_solve_betas(c->stream, w.gmom, w.betas, N));
    }
    HIP_TRY(omc::jump_greeks(c->stream, g, c->ev[5], c->ev[6]));
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    double h[omc::kJumpGreeksQ];
    HIP_TRY(hipMemcpyAsync(h, g.result, sizeof h, hipMemcpyDeviceToHost, c->stream));
    if (betas_out) {
        if (betas) memcpy(betas_out, betas, sizeof(double) * 4 * (size_t)(N + 1));
        else HIP_TRY(hipMemcpyAsync(betas_out, w.betas, sizeof(double) * 4 * (size_t)(N + 1), hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = wait_stream(c))) return rc;

    memset(out, 0, sizeof *out);
    omc_greeks* o = &out->g;
    if (!fit) h[4] = 0.0;  // (no pass 1: the moment table was not written)
    fill_result(&o->base, h, M);
    o->base.folded = 0;
    const double Md = (double)M;
    mean_and_se(h[8], h[9], Md, &o->delta, &o->se_delta);
    mean_and_se(h[10], h[11], Md, &o->gamma, &o->se_gamma);
    if (p->model == OMC_MODEL_GBM) {
        mean_and_se(h[12], h[13], Md, &o->vega, &o->se_vega);
        mean_and_se(h[14], h[15], Md, &o->rho, &o->se_rho);
        mean_and_se(h[16], h[17], Md, &o->theta, &o->se_theta);
        mean_and_se(h[20], h[21], Md, &out->epsilon, &out->se_epsilon);
        mean_and_se(h[24], h[25], Md, &out->dlambda, &out->se_dlambda);
        mean_and_se(h[26], h[27], Md, &out->dmu_j, &out->se_dmu_j);
        mean_and_se(h[28], h[29], Md, &out->dsigma_j, &out->se_dsigma_j);
        mean_and_se(h[30], h[31], Md, &out->theta_score, &out->se_theta_score);
        if (j->lambda == 0.0) out->dlambda = out->se_dlambda = NAN;  // the score is undefined at 0
    } else {  // the sweep carries no tangent to the variance path's parameters
        o->vega = o->rho = o->theta = out->epsilon = NAN;
        o->se_vega = o->se_rho = o->se_theta = out->se_epsilon = NAN;
        out->dlambda = out->dmu_j = out->dsigma_j = out->theta_score = NAN;
        out->se_dlambda = out->se_dmu_j = out->se_dsigma_j = out->se_theta_score = NAN;
    }
    o->bump = bump;
    o->price_up = h[5] / Md;
    o->price_down = h[6] / Md;
    o->n_exercised_up = (int64_t)llround(h[18]);
    o->n_exercised_down = (int64_t)llround(h[19]);
    out->kappa = t.kappa;
    out->drift_rate = t.drift_rate;
    out->n_jumps = (int64_t)llround(h[22]);
    // no pass 2 (ev[5] .. ev[6] is the Greeks sweep), and with the caller's fits neither paths nor pass 1
    if ((rc = read_kernel_times(c->ev, nullptr, &o->base))) return rc;
    float ms = 0;
    if (fit) {
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[1], c->ev[4]));
        o->base.ms_pass1 = ms;
    }
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[5], c->ev[6]));
    o->ms_greeks = ms;
    return 0;
}
