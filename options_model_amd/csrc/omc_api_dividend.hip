// omc_api_dividend.hip -- American options on a stock that pays dividends (include/omc.h): a
// continuous yield q and discrete cash / proportional dividends.  The yield only changes the drift of the paths (r - q;
// discounting stays at r), so a yield-only pricing is omc_price_american's own machinery with that rate on the generator
// and fold-table side.  Discrete dividends go through the dividend generator (omc_dividend.hip), which writes the
// full-storage matrix with ex-dividend spots on the dividend steps; the unchanged two-pass flow (enqueue_lsm) prices it.
#include <algorithm>

#include "omc_ctx.h"
#include "omc_dividend.h"

using namespace omc::abi;

namespace {

// The argument checks of both entry points and the per-step table: mul / cash / has [n_steps + 1] (1 / 0 / 0 where no
// dividend goes ex), composed in float64 in step order, input order within a step.
int compose_schedule(const omc_params* p, double q, const omc_dividend* d, int n_div, std::vector<float>* mul,
                     std::vector<float>* cash, std::vector<int32_t>* has)
{
    int rc;
    if ((rc = check_params(p))) return rc;
    if (!std::isfinite(q)) return fail(-17, "dividend yield q must be finite.");
    if (n_div < 0) return fail(-18, "n_div must be non-negative.");
    if (n_div > 0 && !d) return fail(-19, "null dividend list with n_div > 0.");
    for (int i = 0; i < n_div; ++i) {
        if (!(d[i].t > 0.0 && d[i].t <= p->T)) return fail(-20, "a dividend's time must lie in (0, T].");
        if (!(std::isfinite(d[i].amount) && d[i].amount >= 0.0)) return fail(-21, "a dividend's amount must be finite and non-negative.");
        if (d[i].kind != OMC_DIV_PROPORTIONAL && d[i].kind != OMC_DIV_CASH) return fail(-23, "unknown dividend kind.");
        if (d[i].kind == OMC_DIV_PROPORTIONAL && !(d[i].amount < 1.0)) return fail(-22, "a proportional dividend must be below 1.");
    }
    if (!p->antithetic) return fail(-24, "dividend paths are antithetic pairs (antithetic = 1).");
    if (p->semantics != OMC_SEM_TWO_PASS) return fail(-11, "dividends are priced by the two-pass flow (semantics 2).");
    const int N = p->n_steps;
    std::vector<std::pair<int, int>> order((size_t)n_div);  // (ex-dividend step, input index)
    for (int i = 0; i < n_div; ++i) {
        const int k = (int)std::ceil(d[i].t * N / p->T - 1e-9);
        order[(size_t)i] = {std::min(std::max(k, 1), N), i};
    }
    std::stable_sort(order.begin(), order.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    mul->assign((size_t)N + 1, 1.0f);
    cash->assign((size_t)N + 1, 0.0f);
    has->assign((size_t)N + 1, 0);
    for (size_t j = 0; j < order.size();) {
        const int k = order[j].first;
        double m = 1.0, c = 0.0;
        for (; j < order.size() && order[j].first == k; ++j) {
            const omc_dividend& e = d[order[j].second];
            if (e.kind == OMC_DIV_PROPORTIONAL) {
                m *= 1.0 - e.amount;
                c *= 1.0 - e.amount;
            } else {
                c += e.amount;
            }
        }
        (*mul)[(size_t)k] = (float)m;
        (*cash)[(size_t)k] = (float)c;
        (*has)[(size_t)k] = 1;
    }
    return 0;
}

}  // namespace

extern "C" {

int omc_dividend_schedule(const omc_params* p, double q, const omc_dividend* d, int n_div, float* mul, float* cash,
                          int32_t* has)
{
    std::vector<float> m, c;
    std::vector<int32_t> h;
    int rc;
    if ((rc = compose_schedule(p, q, d, n_div, &m, &c, &h))) return rc;
    if (mul) memcpy(mul, m.data(), sizeof(float) * m.size());
    if (cash) memcpy(cash, c.data(), sizeof(float) * c.size());
    if (has) memcpy(has, h.data(), sizeof(int32_t) * h.size());
    return 0;
}

int omc_price_american_div(omc_ctx* c, const omc_params* p, double q, const omc_dividend* d, int n_div,
                           omc_div_result* out, float* S_keep, int64_t ld)
{
    int rc;
    if ((rc = S_keep ? bind_in(c) : bind(c))) return rc;
    if (!out) return fail(-7, "null result pointer.");
    std::vector<float> mul, cash;
    std::vector<int32_t> has;
    if ((rc = compose_schedule(p, q, d, n_div, &mul, &cash, &has))) return rc;
    if (c->distributed()) return fail(-10, "dividend pricing runs on one GPU.");
    const int N = p->n_steps;
    omc_params gen = *p;  // the generator / fold-table side drifts at r - q; the sweeps discount at p->r
    gen.r = p->r - q;
    memset(out, 0, sizeof *out);
    if (n_div == 0) {  // yield only: omc_price_american's kernels and storage rule
        if ((rc = price_fused(c, p, &gen, &out->base, S_keep, ld))) return rc;
        out->ms_div_paths = out->base.ms_paths;
        return 0;
    }
    // the dividend steps in step order + the closing entry; the image outlives the asynchronous copy (h_table)
    size_t n_ent = 0;
    for (int k = 1; k <= N; ++k) n_ent += has[(size_t)k] ? 1 : 0;
    c->h_table.resize(sizeof(omc::DivEntry) * (n_ent + 1));
    omc::DivEntry* tab = (omc::DivEntry*)c->h_table.data();
    int first = 0;
    for (int k = 1, j = 0; k <= N; ++k) {
        if (!has[(size_t)k]) continue;
        if (!first) first = k;
        tab[j++] = omc::DivEntry{k, mul[(size_t)k], cash[(size_t)k], 0};
    }
    tab[n_ent] = omc::DivEntry{omc::kDivNoStep, 1.0f, 0.0f, 0};
    if ((rc = c->div_tab.ensure(c->h_table.size()))) return rc;
    float* S;
    if ((rc = take_full_matrix(c, p, S_keep, &S, &ld))) return rc;
    const omc::DividendGen g{path_spec(c, p, gen.r, S, ld), (const omc::DivEntry*)c->div_tab.p};
    // (the table's copy stays ahead of event 0: ms_div_paths is the generator alone)
    HIP_TRY(hipMemcpyAsync(c->div_tab.p, tab, c->h_table.size(), hipMemcpyHostToDevice, c->stream));
    if ((rc = enqueue_generated(c, p, S, ld, [&](hipStream_t st) { return omc::launch_dividend_paths(st, g); }))) return rc;
    if ((rc = finish_generated(c, p, &out->base))) return rc;
    out->ms_div_paths = out->base.ms_paths;
    out->n_div_steps = (int32_t)n_ent;
    out->first_div_step = first;
    return 0;
}

}  // extern "C"
