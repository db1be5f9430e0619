// adc_interp.h - the per-keyword act of NaiveInterpolationStrategy (adcraft/baselines/interpolated_expectations.py:155-283,
// 370-439) and its cache key, shared by the device kernel (parts/kernel_interp_agent.inc) and the host twin
// adc_interp_act_host (adc_shims.cpp), so that CPU tests run the very code the GPU runs.
//
// Every value is float64 in numpy's own operation order (build with -ffp-contract=off: no fma is meant here):
//   smoothed()      np.convolve(v, bartlett(min(5, max(1, n-1))) / sum, "same"): identity for n <= 4, .5 v[i-1] + .5 v[i]
//                   for n = 5, (.25 v[i-1] + .5 v[i]) + .25 v[i+1] for n >= 6 (edges drop the missing terms)
//   np.interp       exact hits return the point itself; otherwise slope * (x - x[j]) + y[j]
//   np.sum          pairwise: 0 + blocks of <= 128 summed by 8 accumulators, halves split at a multiple of 8
//   rng.choice(p)   cdf = left-to-right cumsum of p, cdf /= cdf[-1], index = first i with cdf[i] > u
#pragma once
#include "adc_law.h"

#if defined(__HIPCC__)
#define ADC_HD_MEMBER __host__ __device__ __forceinline__
#else
#define ADC_HD_MEMBER inline        // (ADC_HD is `static` on a plain host build: not for member functions)
#endif

namespace adc {

constexpr int kInterpCents = 300;          // the keys cache_to_bid_interpolation_points looks up: np.arange(0.01, 3.01, 0.01)
constexpr int kInterpMaxBids = 2048;       // longest allowed_bids grid the engine takes

// np.arange(0.01, 3.01, 0.01)[c - 1]: numpy fills an arange as start + i * ((start + step) - start)
ADC_HD double interp_cent_x(int c) { return 0.01 + (double)(c - 1) * 0.01; }

// bidstr(bid) = str(round(float(float32 bid), 2)) as cents: 100 x is exact in float64 (24 + 7 significant bits), rint rounds
// half to even on that exact value, as Python's correctly rounded round() does (0.125 -> 0.12)
ADC_HD double interp_key_cents(float bid) { return __builtin_rint(100.0 * (double)bid); }
// float(bidstr(bid)): the double nearest to cents / 100
ADC_HD double interp_key(float bid) { return interp_key_cents(bid) / 100.0; }

// get_expected_rev_per_buyside_click (:178-200)
ADC_HD double interp_erpc(float ave_rpc, int32_t n_rpc, float ave_sctr, int32_t n_sctr)
{
    if (n_rpc < 1 && n_sctr < 1) return 0.3;
    if (n_rpc < 1) return 0.7 * (double)ave_sctr;
    return (double)ave_rpc * (double)ave_sctr;
}

// the acquisition threshold of get_profit_acquisition_function (:377-384)
ADC_HD double interp_threshold(int32_t n_rpc, int32_t n_sctr, double profit_acquisition_threshold)
{
    const double d = (double)(1 + n_rpc) + (double)n_sctr / 5.0;
    return -(1.0 / d) * __builtin_fabs(profit_acquisition_threshold);
}

// end_index = min(L, int(100 * (max_observed + bid_step) - 1)) (:389-391), with Python's slice meaning of a negative value
ADC_HD int interp_end_index(double max_observed, double bid_step, int L)
{
    const double t = __builtin_trunc(100.0 * (max_observed + bid_step) - 1.0);
    if (t >= (double)L) return L;
    if (t >= 0.0) return (int)t;
    const double r = (double)L + t;
    return r > 0.0 ? (int)r : 0;
}

// one series of interpolation points (cents ascending): x = interp_cent_x(cent), y = the cached mean, slot i at i * stride
template <class V>
struct InterpSeries {
    const uint16_t *cent;
    const V *val;
    size_t stride;
    int n;
    ADC_HD_MEMBER double x(int i) const { return interp_cent_x((int)cent[(size_t)i * stride]); }
    ADC_HD_MEMBER double y(int i) const { return (double)val[(size_t)i * stride]; }
};

// smoothed(values)[i] (:203-211)
template <class S>
ADC_HD double interp_smoothed(const S &s, int i)
{
    const int n = s.n;
    if (n <= 4) return s.y(i);
    if (n == 5) return i > 0 ? 0.5 * s.y(i - 1) + 0.5 * s.y(i) : 0.5 * s.y(i);
    double r = i > 0 ? 0.25 * s.y(i - 1) + 0.5 * s.y(i) : 0.5 * s.y(i);
    if (i < n - 1) r = r + 0.25 * s.y(i + 1);
    return r;
}

// np.interp(x, xs, smoothed(ys), left, right) at one x (numpy's arr_interp)
template <class S>
ADC_HD double interp_at(const S &s, double x, double left, double right)
{
    const int n = s.n;
    if (n == 1) {
        const double x0 = s.x(0);
        return x < x0 ? left : (x > x0 ? right : s.y(0));
    }
    if (x > s.x(n - 1)) return right;
    if (x < s.x(0)) return left;
    int lo = 0, hi = n;                      // x(lo) <= x < x(hi) (hi == n: past the end)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (s.x(mid) <= x) lo = mid; else hi = mid;
    }
    const double yj = interp_smoothed(s, lo);
    if (lo == n - 1 || s.x(lo) == x) return yj;
    const double yk = interp_smoothed(s, lo + 1);
    const double xj = s.x(lo), xk = s.x(lo + 1);
    const double slope = (yk - yj) / (xk - xj);
    double r = slope * (x - xj) + yj;
    if (r != r) {
        r = slope * (x - xk) + yk;
        if (r != r && yj == yk) r = yj;
    }
    return r;
}

struct InterpPoint { double margin, cost; };

// get_expected_profit_per_bid_from_cache (:238-283) at one allowed bid; cpc_right = max of the raw cpc means
template <class SC, class SP>
ADC_HD InterpPoint interp_point(const SC &clk, const SP &cpc, double cpc_right, double erpc, double x)
{
    double c, cl;
    if (cpc.n == 0) {
        c = 0.9 * x;
        cl = 1.0;
    } else {
        c = interp_at(cpc, x, 0.01, cpc_right);
        cl = interp_at(clk, x, clk.y(0), clk.y(clk.n - 1));
    }
    const double w = 0.01 + cl;
    return InterpPoint{(-c + erpc) * w, c * w};
}

// numpy's pairwise sum of n values fed in order (np.sum: 0.0 + pairwise_sum(a, n)), streaming: leaves of <= 128 values are
// summed as numpy does (< 8: left to right; else 8 accumulators, combined as a tree, then the rest left to right), a larger
// block splits at n2 = n / 2 rounded down to a multiple of 8.  The open right halves sit in a 5-deep stack (n <= 2048 needs 5),
// shifted rather than indexed so that it stays in registers.
struct PairwiseSum {
    int leaf, fed;                 // size of the leaf being fed, values fed into it
    double r0, r1, r2, r3, r4, r5, r6, r7, res;
    int depth;
    int rs0, rs1, rs2, rs3, rs4;   // right sibling sizes (0: that right half is being fed, its left sum is in ls)
    double ls0, ls1, ls2, ls3, ls4;
    double total;

    ADC_HD_MEMBER void descend(int n)
    {
        while (n > 128) {
            int n2 = n / 2;
            n2 -= n2 % 8;
            rs4 = rs3; rs3 = rs2; rs2 = rs1; rs1 = rs0; rs0 = n - n2;
            ls4 = ls3; ls3 = ls2; ls2 = ls1; ls1 = ls0; ls0 = 0.0;
            ++depth;
            n = n2;
        }
        leaf = n;
        fed = 0;
        res = 0.0;
    }
    ADC_HD_MEMBER void begin(int n)
    {
        depth = 0;
        rs0 = rs1 = rs2 = rs3 = rs4 = 0;
        ls0 = ls1 = ls2 = ls3 = ls4 = 0.0;
        r0 = r1 = r2 = r3 = r4 = r5 = r6 = r7 = 0.0;
        total = 0.0;
        if (n > 0) descend(n);
        else leaf = -1;
    }
    ADC_HD_MEMBER void add(double v)
    {
        const int i = fed++;
        if (leaf < 8) res += v;
        else if (i < leaf - leaf % 8) {
            // accumulator i % 8 is r0 after rotating: first block sets, later blocks add
            const double t = i < 8 ? v : r0 + v;
            r0 = r1; r1 = r2; r2 = r3; r3 = r4; r4 = r5; r5 = r6; r6 = r7; r7 = t;
            if (i + 1 == leaf - leaf % 8) res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
        } else res += v;
        if (fed < leaf) return;
        double s = res;                   // a finished leaf: climb while right halves are complete
        while (depth > 0) {
            if (rs0 > 0) {                // the left half just finished: keep it, feed the right one
                const int n = rs0;
                rs0 = 0;
                ls0 = s;
                descend(n);
                return;
            }
            s = ls0 + s;
            rs0 = rs1; rs1 = rs2; rs2 = rs3; rs3 = rs4; rs4 = 0;
            ls0 = ls1; ls1 = ls2; ls2 = ls3; ls3 = ls4; ls4 = 0.0;
            --depth;
        }
        total = 0.0 + s;
        leaf = -1;
    }
};

// the keyword's act: mass, draw and pick over allowed_bids[0, end).  `eval(j)` returns interp_point at grid[j].
// Result: index -1 when mass <= 0 (no draw), else rng.choice's index for uniform u (asked for only then).
struct InterpPick { int index; double mass; };
template <class Eval, class Uniform>
ADC_HD InterpPick interp_pick(const Eval &eval, double thr, int end, const Uniform &uniform)
{
    PairwiseSum pw;
    pw.begin(end);
    for (int j = 0; j < end; ++j) {
        const double m = eval(j).margin;
        pw.add((m > thr ? m : thr) - thr);          // np.maximum(margin, thr) - thr
    }
    const double mass = end > 0 ? pw.total : 0.0;
    if (!(mass > 0.0)) return InterpPick{-1, mass};
    const double u = uniform();
    double last = 0.0;                              // cdf[-1]: the zeros past end_index add nothing
    for (int j = 0; j < end; ++j) {
        const double m = eval(j).margin;
        last = last + ((m > thr ? m : thr) - thr) / mass;
    }
    double c = 0.0;
    int idx = end - 1;
    for (int j = 0; j < end; ++j) {
        const double m = eval(j).margin;
        c = c + ((m > thr ? m : thr) - thr) / mass;
        if (c / last > u) { idx = j; break; }
    }
    return InterpPick{idx, mass};
}

}  // namespace adc
