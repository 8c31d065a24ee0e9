// omc_crit.h -- per-step exercise tables of pass 2: the exact float32 spots at which a fixed float64 decision switches.
//
// At step t pass 2 decides for every loaded float32 spot s whether a path exercises; with the step's fits (b0, b1, b2)
// and cK[t] fixed that decision is a function of s alone.  In exact arithmetic it is
//      pay(u) > 0  and  pay(u) > b0 + b1 u + b2 u^2,   pay(u) = -K u (put) / K u (call),
// with u the path's moneyness: u = s / K - 1 for the stored path, u = cK[t] / s - 1 for its folded partner -- a quadratic
// in a quantity monotone in s, cut by a half-line, so the spots that exercise form at most two intervals.  On the
// float32 grid the endpoints are found by evaluating the DECISION ITSELF (the caller's predicate: the float64 expressions
// of the sweep, verbatim) at float32 ordinals around the roots of that quadratic; afterwards a sweep decides a spot with
// one unsigned subtract and compare per interval on its bit pattern.
//
// Domain: the non-negative floats, bit patterns 0 .. 0x7f800000 (+inf), whose unsigned order is their order.  A bit
// pattern above that (a negative float, a NaN) is in no interval.
//
// A step is IRREGULAR (the sweep then decides it with the float64 code) when a fit is non-finite other than "no fit",
// two roots nearly coincide, a linear fit's slope nearly cancels the payoff's, a window around a candidate holds more than one switch, the sampled regions between
// windows are not constant or do not join their windows, or more than two intervals come out.
//
// Host and device: crit_mask64 evaluates 64 ordinals -- one per lane on the device, a loop on the host -- so the same
// builder runs in the sweep's table kernel and in the CPU tests.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define OMC_HD __host__ __device__
#else
#define OMC_HD
#endif

namespace omc {

constexpr uint32_t kCritTop = 0x7f800000u;  // +inf: the last ordinal of the domain
constexpr int kCritHalf = 32;               // a candidate's window: ordinals [o - 32, o + 32)
constexpr int kCritMaxCand = 6;
constexpr uint32_t kCritIrregular = 0xffffffffu;  // lo[0] of an irregular step (a real lo is <= kCritTop)

// decisions of one path kind at one step: spot bits b exercise iff crit_in(lo[0], lo[1], len[0], len[1], b)
struct CritIv {
    uint32_t lo[2], len[2];
};

// the table test: (b - lo) < len (unsigned) holds exactly for b in [lo, lo + len); `|`, not `||`, keeps it branch-free
OMC_HD inline bool crit_in(uint32_t lo0, uint32_t lo1, uint32_t len0, uint32_t len1, uint32_t b)
{
    return ((b - lo0) < len0) | ((b - lo1) < len1);
}

OMC_HD inline float crit_float(uint32_t o) { return __builtin_bit_cast(float, o); }
OMC_HD inline uint32_t crit_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

// bit i of the result = pred(ord(i)), i = 0 .. 63
template <class P, class O>
OMC_HD inline uint64_t crit_mask64(const P& pred, const O& ord)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int i = (int)(threadIdx.x & 63);
    return __builtin_amdgcn_ballot_w64(pred(crit_float(ord(i))));
#else
    uint64_t m = 0;
    for (int i = 0; i < 64; ++i) m |= (uint64_t)(pred(crit_float(ord(i))) ? 1 : 0) << i;
    return m;
#endif
}

// Candidate spots of one path kind: the ends of the domain, where pay(u) = 0 and where the quadratic has its roots,
// mapped from u to s.
// kind 0: u = s / K - 1 (stored path); kind 1: u = ck / s - 1 (folded partner).  Returns the number written to cand,
// or -1 if the step is irregular.
OMC_HD inline int crit_candidates(int kind, int is_put, double K, double ck, double b0, double b1, double b2,
                                  double (&cand)[kCritMaxCand])
{
    int n = 0;
    auto add_u = [&](double u) {
        double s;
        if (kind == 0) s = K * (1.0 + u);
        else s = (1.0 + u) > 0.0 ? ck / (1.0 + u) : -1.0;
        if (s >= 0.0 && n < kCritMaxCand) cand[n++] = s;  // also drops NaN
    };
    // the ends of the domain: 0 and +inf, where the partner's 1 / s and the products with an infinite u are not the
    // limits of their neighbours' values
    cand[n++] = 0.0;
    cand[n++] = __builtin_huge_val();
    add_u(0.0);
    if (b0 == __builtin_huge_val() && b1 == 0.0 && b2 == 0.0) return n;  // no fit: the continuation value is +inf
    if (!isfinite(b0) || !isfinite(b1) || !isfinite(b2)) return -1;
    // pay(u) - cont(u) = -(A u^2 + B u + C)
    const double A = b2, B = b1 - (is_put ? -K : K), C = b0;
    if (A == 0.0) {
        // a slope that is nearly zero next to its terms: rounding could flip the decision far from -C / B
        if (fabs(B) <= 1e-9 * (fabs(b1) + K)) return -1;
        add_u(-C / B);
        return n;
    }
    const double disc = B * B - 4.0 * A * C;
    const double scale = B * B + fabs(4.0 * A * C);
    if (fabs(disc) <= 1e-9 * scale) return -1;  // a (nearly) double root: no certified switch
    if (disc < 0.0) return n;
    const double q = -0.5 * (B + copysign(sqrt(disc), B));
    add_u(q / A);
    if (q != 0.0) add_u(C / q);
    return n;
}

// The intervals of pred over the domain from the candidate spots; false = irregular.
template <class P>
OMC_HD inline bool crit_build(const P& pred, const double* cand, int ncand, CritIv& out)
{
    out.lo[0] = out.lo[1] = out.len[0] = out.len[1] = 0;
    // windows around the candidates, sorted and merged when they touch
    uint32_t wa[kCritMaxCand], wb[kCritMaxCand];  // [wa, wb] inclusive
    int nw = 0;
    for (int i = 0; i < ncand; ++i) {
        const double s = cand[i];
        const uint32_t o = s >= 3.4028234663852886e38 ? kCritTop : crit_bits((float)s);
        const uint32_t a = o > (uint32_t)kCritHalf ? o - kCritHalf : 0u;
        const uint32_t b = o + kCritHalf - 1 < kCritTop ? o + kCritHalf - 1 : kCritTop;
        int k = nw++;
        while (k > 0 && wa[k - 1] > a) {
            wa[k] = wa[k - 1];
            wb[k] = wb[k - 1];
            --k;
        }
        wa[k] = a;
        wb[k] = b;
    }
    int m = 0;
    for (int i = 0; i < nw; ++i) {
        if (m > 0 && wa[i] <= wb[m - 1] + 1) {
            if (wb[i] > wb[m - 1]) wb[m - 1] = wb[i];
        } else {
            wa[m] = wa[i];
            wb[m] = wb[i];
            ++m;
        }
    }
    nw = m;
    // walk the domain: gaps are sampled (64 ordinals, both ends included), windows evaluated ordinal by ordinal
    int nint = 0;
    bool cur = false, have = false;  // value at the last ordinal seen
    uint32_t start = 0;
    auto set = [&](bool v, uint32_t o) -> bool {  // the value becomes v at ordinal o
        if (have && v == cur) return true;
        if (v) start = o;
        else if (have) {
            if (nint == 2) return false;
            out.lo[nint] = start;
            out.len[nint] = o - start;
            ++nint;
        }
        cur = v;
        have = true;
        return true;
    };
    uint32_t next = 0;  // first ordinal not yet covered
    for (int w = 0; w <= nw; ++w) {
        const uint32_t g0 = next, g1e = w < nw ? wa[w] : kCritTop + 1;  // gap [g0, g1e)
        if (g1e > g0) {
            const uint64_t span = (uint64_t)(g1e - 1 - g0);
            const uint64_t mk = crit_mask64(pred, [&](int i) { return (uint32_t)(g0 + span * (uint64_t)i / 63u); });
            if (mk != 0 && mk != ~0ull) return false;
            const bool v = mk != 0;
            if (have && v != cur) return false;  // a gap must continue the window on its left
            if (!set(v, g0)) return false;
        }
        if (w == nw) break;
        int switches = 0;
        for (uint32_t c0 = wa[w]; c0 <= wb[w]; c0 += 64) {
            const uint32_t c1 = wb[w] - c0 >= 63 ? c0 + 63 : wb[w];
            const int n = (int)(c1 - c0) + 1;
            const uint64_t valid = n == 64 ? ~0ull : (1ull << n) - 1;
            const uint64_t mk = crit_mask64(pred, [&](int i) { return c0 + (uint32_t)i <= c1 ? c0 + (uint32_t)i : c1; }) & valid;
            // bit i of d: the value at c0 + i differs from the one before it (the first ordinal of the walk always counts)
            const uint64_t prev = have ? (uint64_t)cur : (~mk & 1u);
            uint64_t d = (mk ^ ((mk << 1) | prev)) & valid;
            while (d) {
                const int i = __builtin_ctzll(d);
                d &= d - 1;
                // one switch per candidate window; a merged window may hold as many as it has candidates
                if (have && ++switches > ncand) return false;
                if (!set((mk >> i) & 1u, c0 + (uint32_t)i)) return false;
            }
            if (c1 == wb[w]) break;
        }
        next = wb[w] + 1;  // the gap on the right must continue the window's last value: checked when it is visited
    }
    if (cur) {
        if (nint == 2) return false;
        out.lo[nint] = start;
        out.len[nint] = kCritTop + 1 - start;
        ++nint;
    }
    return true;
}

OMC_HD inline bool crit_in(const CritIv& t, uint32_t b) { return crit_in(t.lo[0], t.lo[1], t.len[0], t.len[1], b); }

}  // namespace omc
