// omc_api_dividend_bounds.hip -- Andersen-Broadie price bounds of American options on a stock that pays discrete
// dividends, and the dividend generator as an entry point of its own (include/omc_dividend_bounds.h, DESIGN.md section
// 29): omc_price_american_bounds' flow (run_bounds, omc_api_bounds.hip) with the dividend generator (omc_dividend.hip; with
// the variance kept: omc_dividend_bounds.hip) writing the matrices and the kernels of omc_dividend_bounds.hip simulating
// the fresh paths from the outer spot (GBM) or (spot, variance) state (Heston) AND from the date.  A call without a
// dividend takes the same route: its table holds the closing entry alone, no step has a dividend, and every spot carries
// the vanilla generator's bits.
#include "../../include/omc_dividend_bounds.h"
#include "omc_ctx.h"
#include "omc_dividend_bounds.h"

using namespace omc::abi;

namespace {

// The argument checks (the omc_params checks, -17 .. -24: omc_dividend_schedule's) and the per-step table.  The two-pass
// pricing's semantics check (-11) is not one of them: p->semantics is not used.  start_state: p->v0 of Heston schemes
// 0 .. 2 is a stored state and is not validated, and p->S0 may be 0.
int compose(const omc_params* p, double q, const omc_dividend* d, int n_div, bool start_state, std::vector<float>* mul,
            std::vector<float>* cash, std::vector<int32_t>* has)
{
    int rc;
    if (!p) return fail(-7, "null params.");
    omc_params chk = *p;
    if (start_state && p->model == OMC_MODEL_HESTON && p->heston_scheme != OMC_HESTON_QE) chk.v0 = 0.0;
    if (start_state && p->S0 == 0.0) chk.S0 = 1.0;  // a spot that a cash dividend has taken to 0 is a state too
    if (p->semantics >= 0 && p->semantics <= 2) chk.semantics = OMC_SEM_TWO_PASS;  // (an unknown one stays: -4)
    if ((rc = check_params(&chk))) return rc;  // (sizes first: the table has n_steps + 1 rows)
    const size_t n = (size_t)p->n_steps + 1;
    mul->resize(n);
    cash->resize(n);
    has->resize(n);
    return omc_dividend_schedule(&chk, q, d, n_div, mul->data(), cash->data(), has->data());
}

// The call's tables in the context's device buffer: [entries + the closing one | first_after [N+1]].  room() makes the
// buffer large enough (no launch); upload() copies the images and returns when they are copied (they are the caller's
// pageable memory).
struct DeviceTables {
    const std::vector<omc::DivEntry>& tab;
    const std::vector<omc::DivStart>& first;
    size_t b_tab() const { return sizeof(omc::DivEntry) * tab.size(); }
    size_t b_first() const { return sizeof(omc::DivStart) * first.size(); }
    int room(omc_ctx* c) const { return c->div_tab.ensure(b_tab() + b_first()); }
    hipError_t upload(omc_ctx* c, const omc::DivEntry** d_tab, const omc::DivStart** d_first) const
    {
        char* b = (char*)c->div_tab.p;
        hipError_t e = hipMemcpyAsync(b, tab.data(), b_tab(), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && b_first())
            e = hipMemcpyAsync(b + b_tab(), first.data(), b_first(), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return e;
        *d_tab = (const omc::DivEntry*)b;
        if (d_first) *d_first = (const omc::DivStart*)(b + b_tab());
        return hipSuccess;
    }
};

}  // namespace

extern "C" int omc_dividend_paths_f32(omc_ctx* c, const omc_params* p, double q, const omc_dividend* d, int n_div,
                                      int step_offset, float* S, float* V, int64_t ld)
{
    int rc;
    if ((rc = bind_in(c))) return rc;
    std::vector<float> mul, cash;
    std::vector<int32_t> has;
    if ((rc = compose(p, q, d, n_div, true, &mul, &cash, &has))) return rc;
    if ((rc = check_matrix(S, ld, p->n_paths))) return rc;
    if (V && p->model != OMC_MODEL_HESTON) return fail(-7, "a variance matrix is kept under Heston only (V must be NULL).");
    if (step_offset < 0 || step_offset > p->n_steps) return fail(-41, "step_offset must lie in [0, n_steps].");
    std::vector<omc::DivEntry> tab;
    omc::dividend_tables(p->n_steps, mul.data(), cash.data(), has.data(), step_offset, &tab, nullptr);
    const omc::DivEntry* d_tab = nullptr;
    const std::vector<omc::DivStart> none;
    const DeviceTables dt{tab, none};
    if ((rc = dt.room(c))) return rc;
    HIP_TRY(dt.upload(c, &d_tab, nullptr));
    const omc::DividendGen g{path_spec(c, p, p->r - q, S, ld), d_tab};
    HIP_TRY(V ? omc::launch_dividend_paths_sv(c->stream, g, V) : omc::launch_dividend_paths(c->stream, g));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int omc_price_american_bounds_div(omc_ctx* c, const omc_params* p, double q, const omc_dividend* d, int n_div,
                                             const omc_bounds_config* cfg, const double* betas, double* betas_out,
                                             double* q_out, double* samples_out, omc_bounds* out)
{
    int rc;
    if ((rc = bind(c))) return rc;
    if (!cfg || !out) return fail(-7, "null bounds config or result pointer.");
    std::vector<float> mul, cash;
    std::vector<int32_t> has;
    if ((rc = compose(p, q, d, n_div, false, &mul, &cash, &has))) return rc;
    const bool heston = p->model == OMC_MODEL_HESTON;
    if (heston && p->heston_scheme != OMC_HESTON_REFERENCE_CLAMP && p->heston_scheme != OMC_HESTON_FULL_TRUNCATION)
        return fail(-12, "price bounds with dividends take the reference or the full-truncation Heston scheme, not the "
                         "calibrator's or QE.");
    if (cfg->regressors != 0) return fail(-4, "the dividend bounds take a policy on the spot alone (regressors 0).");
    const double rq = p->r - q;
    std::vector<omc::DivEntry> tab;
    std::vector<omc::DivStart> first;
    omc::dividend_tables(p->n_steps, mul.data(), cash.data(), has.data(), 0, &tab, &first);
    omc::BoundsArgs a{};
    omc::DividendBoundsLaw l{{heston ? 1 : 0, p->heston_scheme, rq, p->sigma, p->T, p->v0, p->kappa, p->theta, p->xi, p->rho,
                              nullptr}, nullptr, nullptr};
    // the tables go to the device with the first hook that enqueues work: a refusal of run_bounds launches nothing
    const DeviceTables dt{tab, first};
    if ((rc = dt.room(c))) return rc;
    auto tables = [&]() { return l.tab ? hipSuccess : dt.upload(c, &l.tab, &l.first); };
    BoundsFlow f;
    one_asset_flow(f, a, l, l.d, p, cfg);
    f.fit_paths = [&](float* S, int64_t ld) -> int {
        HIP_TRY(tables());
        HIP_TRY(omc::launch_dividend_paths(c->stream, omc::DividendGen{path_spec(c, p, rq, S, ld), l.tab}));
        return 0;
    };
    // (a given policy has no fit: the lower sweep is then the first hook that enqueues work)
    f.lower = [&, lower = f.lower](hipStream_t st, double* res) {
        const hipError_t e = tables();
        return e != hipSuccess ? e : lower(st, res);
    };
    f.outer = [&](hipStream_t st) {  // the outer paths: spots and, under Heston, the variance state, KEEP
        const omc::DividendGen g{path_spec(c, p, rq, (float*)a.So, a.n_outer, a.n_outer, cfg->stream_outer, 0), l.tab};
        return heston ? omc::launch_dividend_paths_sv(st, g, (float*)l.d.Vo) : omc::launch_dividend_paths(st, g);
    };
    return run_bounds(c, p, cfg, betas, betas_out, q_out, samples_out, out, f);
}
