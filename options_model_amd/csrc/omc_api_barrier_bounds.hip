// omc_api_barrier_bounds.hip -- Andersen-Broadie price bounds of American barrier options, and the barrier generator that
// keeps its paths' state as an entry point of its own (include/omc_barrier_bounds.h):
// omc_price_american_bounds' flow (run_bounds, omc_api_bounds.hip) with the barrier generator writing the matrices -- the
// ENCODED one the policy is fitted on and the walk reads, and beside it the outer paths' real spots, variance state and
// first-hit steps -- and the kernels of omc_barrier_bounds.hip simulating the fresh paths from that state.
#include "../../include/omc_barrier_bounds.h"
#include "omc_barrier_bounds.h"
#include "omc_ctx.h"

using namespace omc::abi;

namespace {

// The contract's checks, in omc_price_barrier's order, for the models that have kernels here.  state_v0: p->v0 of a Heston
// call is a stored state and is not validated; state_s0: the paths restart from a state that has been hit, S0 may lie
// beyond the barrier.
int check_contract(const omc_params* p, const omc_barrier* b, bool state_v0, bool state_s0, omc::BarrierTest* test)
{
    int rc;
    if (!p) return fail(-7, "null params.");
    if (!b) return fail(-7, "null barrier pointer.");
    omc_params chk = *p;
    if (state_v0 && p->model == OMC_MODEL_HESTON && p->heston_scheme != OMC_HESTON_QE) chk.v0 = 0.0;
    if (p->semantics >= 0 && p->semantics <= 2) chk.semantics = OMC_SEM_TWO_PASS;  // (an unknown one stays: -4)
    if ((rc = check_params(&chk))) return rc;
    if (b->kind < OMC_BARRIER_DOWN_OUT || b->kind > OMC_BARRIER_UP_IN || b->monitoring < OMC_MONITOR_DISCRETE ||
        b->monitoring > OMC_MONITOR_CONTINUOUS)
        return fail(-15, "unknown barrier kind or monitoring.");
    if (!p->antithetic) return fail(-15, "barrier paths are antithetic pairs (antithetic = 1).");
    if (b->monitoring == OMC_MONITOR_CONTINUOUS)
        return fail(-12, "the barrier price bounds take discrete monitoring (the Brownian-bridge draw is no state of the path).");
    if (p->model == OMC_MODEL_HESTON && p->heston_scheme != OMC_HESTON_REFERENCE_CLAMP &&
        p->heston_scheme != OMC_HESTON_FULL_TRUNCATION)
        return fail(-12, "the barrier price bounds take the reference or the full-truncation Heston scheme, not the "
                         "calibrator's or QE.");
    if (!(std::isfinite(b->H) && b->H > 0.0)) return fail(-13, "barrier H must be finite and positive.");
    const int up = (b->kind == OMC_BARRIER_UP_OUT || b->kind == OMC_BARRIER_UP_IN) ? 1 : 0;
    const int knock_in = (b->kind == OMC_BARRIER_DOWN_IN || b->kind == OMC_BARRIER_UP_IN) ? 1 : 0;
    *test = omc::barrier_test(p->K, p->is_put ? 1 : 0, b->H, up, knock_in);
    if (!state_s0) {
        const float thr = omc::barrier_threshold(b->H, up), s0f = (float)p->S0;
        if (up ? (p->S0 >= b->H || s0f >= thr) : (p->S0 <= b->H || s0f <= thr))
            return fail(-14, "S0 lies on or beyond the barrier (the option is already knocked).");
    }
    return 0;
}

}  // namespace

extern "C" int omc_barrier_paths_state_f32(omc_ctx* c, const omc_params* p, const omc_barrier* b, int start_hit, float* E,
                                           float* S, float* V, int32_t* hit, int64_t ld)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    if (start_hit != 0 && start_hit != 1) return fail(-15, "start_hit is 0 (not hit) or 1 (hit before the start).");
    omc::BarrierTest test{};
    if ((rc = check_contract(p, b, true, start_hit != 0, &test))) return rc;
    if (c->distributed()) return fail(-10, "the barrier generator runs on one GPU.");
    if ((rc = check_matrix(E, ld, p->n_paths))) return rc;
    if (!S || !hit) return fail(-7, "null spot matrix or hit pointer.");
    const bool heston = p->model == OMC_MODEL_HESTON;
    if (heston != (V != nullptr)) return fail(-7, "the variance matrix is kept under Heston and only there (GBM: V must be NULL).");
    const omc::BarrierStateGen g{path_spec(c, p, p->r, E, ld), test, start_hit, S, V, hit};
    HIP_TRY(omc::launch_barrier_paths_state(c->stream, g));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int omc_price_american_bounds_barrier(omc_ctx* c, const omc_params* p, const omc_barrier* b,
                                                 const omc_bounds_config* cfg, const double* betas, double* betas_out,
                                                 double* q_out, double* samples_out, omc_bounds* out)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!cfg || !out) return fail(-7, "null bounds config or result pointer.");
    omc::BarrierTest test{};
    if ((rc = check_contract(p, b, false, false, &test))) return rc;
    if (cfg->regressors != 0) return fail(-4, "the barrier bounds take a policy on the encoded index alone (regressors 0).");
    if (c->bounds_subopt == 2)
        return fail(-12, "option bounds_suboptimality: a vanilla European value is no bound on a barrier continuation value "
                         "(the payoff check, 1, is taken).");
    if (c->bounds_cv != 0) return fail(-12, "option bounds_control_variate: the barrier bounds have no control variate.");
    const bool heston = p->model == OMC_MODEL_HESTON;
    const int N = p->n_steps;
    const int up = (b->kind == OMC_BARRIER_UP_OUT || b->kind == OMC_BARRIER_UP_IN) ? 1 : 0;
    omc::BoundsArgs a{};
    omc::BarrierBoundsLaw l{{heston ? 1 : 0, p->heston_scheme, p->r, p->sigma, p->T, p->v0, p->kappa, p->theta, p->xi, p->rho,
                             nullptr}, test, nullptr, nullptr,
                            c->bounds_every >= 2 ? omc::bounds_schedule(N, c->bounds_every).k : 0};
    BoundsFlow f;
    one_asset_flow(f, a, l, l.d, p, cfg);
    // the flow's room beside the encoded outer matrix: real spots [N+1][n_outer] | Heston: variance state | hit [n_outer]
    size_t o_v = 0, o_hit = 0;
    if (cfg->n_outer > 0) {  // (sizes are checked in run_bounds, before the room is used)
        const size_t mat = up256(sizeof(float) * (size_t)(N + 1) * (size_t)cfg->n_outer);
        o_v = mat;
        o_hit = o_v + (heston ? mat : 0);
        f.extra_bytes = o_hit + sizeof(int32_t) * (size_t)cfg->n_outer;
    }
    f.bind = [&](const omc::BoundsArgs& common, char* extra) {
        a = common;
        a.s0 = (float)p->S0;  // the generator's start value, so every spot is the generator's
        l.Sr = (const float*)extra;
        l.d.Vo = heston ? (const float*)(extra + o_v) : nullptr;
        l.hit = (const int32_t*)(extra + o_hit);
    };
    // the policy's paths: omc_price_barrier's encoded matrix (its European sums go to the barrier pricing's buffers, unread)
    omc::BarrierGen fit{};
    fit.is_put = p->is_put ? 1 : 0; fit.up = up; fit.knock_in = test.knock_out ? 0 : 1; fit.continuous = 0;
    fit.K = p->K; fit.H = b->H;
    if (cfg->policy != OMC_POLICY_GIVEN) {
        fit.paths = path_spec(c, p, p->r, nullptr, 0);
        if ((rc = c->bar_part.ensure(sizeof(double) * omc::kBarrierQ * (size_t)omc::barrier_blocks(fit)))) return rc;
        if ((rc = c->bar_res.ensure(sizeof(double) * omc::kBarrierQ))) return rc;
    }
    f.fit_paths = [&](float* S, int64_t ld) -> int {
        fit.paths = path_spec(c, p, p->r, S, ld);
        fit.part = (double*)c->bar_part.p;
        fit.result = (double*)c->bar_res.p;
        HIP_TRY(omc::launch_barrier_paths(c->stream, fit));
        return 0;
    };
    f.outer = [&](hipStream_t st) {  // the outer paths: the encoded index, and the state the inner paths start from, KEEP
        const omc::BarrierStateGen g{path_spec(c, p, p->r, (float*)a.So, a.n_outer, a.n_outer, cfg->stream_outer, 0), test, 0,
                                     (float*)l.Sr, (float*)l.d.Vo, (int32_t*)l.hit};
        return omc::launch_barrier_paths_state(st, g);
    };
    // a knock-out's dead items leave through the keep mask and the list-driven sweep (a knock-in has none)
    if (test.knock_out) f.mark_items = [&](hipStream_t st, const omc::BoundsCheck& k) { return omc::barrier_bounds_mark(st, a, l, k); };
    return run_bounds(c, p, cfg, betas, betas_out, q_out, samples_out, out, f);
}
