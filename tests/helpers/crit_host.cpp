// Host build of pass 2's exercise-table builder (options_model_amd/csrc/omc_crit.h) for the CPU tests.  The predicates
// repeat the sweep's float64 decisions; the partner's 1 / S is an IEEE division here where the device seeds a Newton step
// with v_rcp_f64 -- the builder only ever sees the predicate it is given, so what is tested is that it finds that
// predicate's switches exactly.
#include <cmath>
#include <cstdint>

#include "omc_crit.h"

namespace {
struct Pred {
    int kind, is_put;
    double K, invK, ck, b0, b1, b2;
    bool operator()(float s) const
    {
        const double sd = (double)s;
        if (kind == 0) {
            const double imm = is_put ? K - sd : sd - K;
            const double u = std::fma(sd, invK, -1.0);
            const double cont = std::fma(u, std::fma(u, b2, b1), b0);
            return (imm > 0.0) & (imm > cont);
        }
        double r = 1.0 / sd;
        r = std::fma(std::fma(-sd, r, 1.0), r, r);
        const double ub = std::fma(ck, r, -1.0);
        const double immb = is_put ? -K * ub : K * ub;
        const double contb = std::fma(ub, std::fma(ub, b2, b1), b0);
        return (immb > 0.0) & (immb > contb);
    }
};
}  // namespace

extern "C" int crit_host_build(int kind, int is_put, double K, double ck, double b0, double b1, double b2, uint32_t* out)
{
    const Pred p{kind, is_put, K, 1.0 / K, ck, b0, b1, b2};
    double cand[omc::kCritMaxCand];
    const int n = omc::crit_candidates(kind, is_put, K, ck, b0, b1, b2, cand);
    omc::CritIv iv{};
    if (n < 0 || !omc::crit_build(p, cand, n, iv)) return 0;
    out[0] = iv.lo[0]; out[1] = iv.lo[1]; out[2] = iv.len[0]; out[3] = iv.len[1];
    return 1;
}

// decisions of the predicate (pred = 1) or of the table (pred = 0) for n spot bit patterns
extern "C" void crit_host_eval(int kind, int is_put, double K, double ck, double b0, double b1, double b2,
                               const uint32_t* tab, const uint32_t* bits, int64_t n, uint8_t* pred, uint8_t* table)
{
    const Pred p{kind, is_put, K, 1.0 / K, ck, b0, b1, b2};
    omc::CritIv iv{{tab[0], tab[1]}, {tab[2], tab[3]}};
    for (int64_t i = 0; i < n; ++i) {
        pred[i] = p(__builtin_bit_cast(float, bits[i]));
        table[i] = omc::crit_in(iv, bits[i]);
    }
}
