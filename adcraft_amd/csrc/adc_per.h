// adc_per.h - the law of prioritised replay on the device (Schaul, Quan, Antonoglou, Silver 2016, the proportional variant) for
// the off-policy learners of adc_td3.h / adc_sac.h: a radix-64 sum tree over the replay ring's slots that is sampled and updated
// on the device, importance weights for the critics' loss, and the priorities' update from the critics' errors.  Shared by the
// device kernels (parts/kernel_per.inc) and the host twins adc_per_*_host (adc_shims.cpp); tests/per_ref.py restates these
// comments in numpy, bit for bit.
//
// Every float32 value below is the result of ONE correctly rounded IEEE operation (-ffp-contract=off); "f64" marks what is
// computed in float64.  det_log is adc_law.h's, mlp_exp adc_mlp.h's, draw adc_law.h's, the td3 key adc_td3.h's.
//
//   leaves     leaf[C] float32, one per ring slot; slots >= size hold 0.  pa(p) = alpha == 0 ? 1 : mlp_exp(alpha * det_log(p)).
//              A cell `top` (float32, 1.0f at init) is the largest leaf any update has written.  A transition written by a
//              store or a buffer load gets leaf = top, a slot overwritten by the ring's wrap like any new one.
//   tree       radix 64: level 0 is the leaves, level l has n_l = ceil(n_{l-1} / 64) float64 nodes, up to the level L with one
//              node, the root (L = ceil(log64 C), at least 1).  A node's 64 children (absent ones 0, leaves widened to f64) are
//              scanned inclusively by Hillis-Steele over 64 lanes: for s = 1, 2, 4, 8, 16, 32, all lanes at once,
//              c_i = c_i + c_{i-s} for i >= s.  The node's value is c_63 of that scan, so a node and the scan used to descend
//              through it agree by construction.  total = the root.
//   sample     update u, element b: w = draw(td3 key, b / 2, ST_PER_BATCH = 22, 0, u); hi, lo = its words 2 (b % 2),
//              2 (b % 2) + 1; u53 = f64(((hi << 32) | lo) >> 11) * 2^-53; m = u53 * total.  At each node from the root down:
//              child = the first i with c_i > m, or when there is none the last child whose value is nonzero (child 0 when all
//              are zero); m = m - c_{child-1} (nothing subtracted for child 0).  The leaf reached is the slot.  Every stored slot
//              has a positive leaf and every other one 0, so the slot is < size.  Duplicates are plain samples.
//   guard      the lanes of a scan sum in different orders, so c_i can exceed c_{i-1} by an ulp where child i is 0.  So that no
//              draw can leave the arrays: an index past its level's last node is that node, a slot >= size is size - 1.
//   weight     lmin = the smallest sampled leaf of the batch; w_b = beta == 0 ? 1 : mlp_exp(beta * (det_log(lmin) -
//              det_log(leaf_b))) (a difference, a product), in (0, 1]: normalised by the batch's largest weight.
//   critic     d_i = Q_i - y; the output delta is w_b * d_i, the loss piece w_b * (0.5 * (d_i * d_i)).  The actor's step, the
//              temperature's step and the other statistics are unweighted.
//   priority   mm = 0.5f * (|d_1| + |d_2|) from the unweighted d; p = mm + eps; p = p > cap ? cap : p; p = p >= eps ? p : eps
//              (a NaN becomes eps).  A slot's new leaf is the MAXIMUM of pa(p_b) over the batch elements that sampled it;
//              top = max(top, the new leaves).  Then every node on a touched path is recomputed in full from its children, level
//              by level: no delta arithmetic on sums.  The next update's sample reads the new tree.
#pragma once
#include <vector>

#include "adc_td3.h"

namespace adc {

constexpr uint32_t ST_PER_BATCH = 22;
constexpr int kPerRadix = 64, kPerMaxLevels = 6;       // 64^6 slots: more than a ring can hold

struct PerLaw {
    float alpha, beta, eps, cap;
};

// the tree's shape for a ring of C slots: n[0] = C leaves, n[l] nodes at level l, n[levels] = 1
struct PerShape {
    int levels;
    int64_t n[kPerMaxLevels + 1];
};
inline PerShape per_shape_of(int64_t C)
{
    PerShape s{};
    s.n[0] = C;
    int l = 0;
    do {
        s.n[l + 1] = (s.n[l] + kPerRadix - 1) / kPerRadix;
        ++l;
    } while (s.n[l] > 1 && l < kPerMaxLevels);
    s.levels = l;
    return s;
}

ADC_HD float per_pa(float p, float alpha)
{
    if (alpha == 0.0f) return 1.0f;
    const float lg = det_log(p), x = alpha * lg;
    return mlp_exp(x);
}
ADC_HD float per_priority(float d1, float d2, float eps, float cap)
{
    const float a1 = __builtin_fabsf(d1), a2 = __builtin_fabsf(d2);
    const float s = a1 + a2, mm = 0.5f * s;
    float p = mm + eps;
    p = p > cap ? cap : p;
    p = p >= eps ? p : eps;
    return p;
}
ADC_HD float per_weight(float lmin, float leaf, float beta)
{
    if (beta == 0.0f) return 1.0f;
    const float d = det_log(lmin) - det_log(leaf), x = beta * d;
    return mlp_exp(x);
}
ADC_HD double per_u53(uint64_t key, uint32_t b, uint32_t update)
{
    const U4 w = draw(key, b >> 1, ST_PER_BATCH, 0u, update);
    const uint32_t hi = (b & 1u) ? w.z : w.x, lo = (b & 1u) ? w.w : w.y;
    const uint64_t bits = (((uint64_t)hi << 32) | (uint64_t)lo) >> 11;
    return (double)bits * 1.1102230246251565e-16;      // 2^-53
}

// ---- the host's side of the tree ----------------------------------------------------------------------------------------------------
// the inclusive scan of a node's 64 children, in place
inline void per_scan64(double *c)
{
    for (int s = 1; s < kPerRadix; s += s) {
        double t[kPerRadix];
        for (int i = 0; i < kPerRadix; ++i) t[i] = i >= s ? c[i] + c[i - s] : c[i];
        for (int i = 0; i < kPerRadix; ++i) c[i] = t[i];
    }
}
// the child a descent with m takes in a node: v the children's values, c their scan; m becomes the child's
inline int per_pick(const double *v, const double *c, double &m)
{
    int child = -1;
    for (int i = 0; i < kPerRadix && child < 0; ++i)
        if (c[i] > m) child = i;
    if (child < 0) {
        child = 0;
        for (int i = 0; i < kPerRadix; ++i)
            if (v[i] != 0.0) child = i;
    }
    if (child > 0) m = m - c[child - 1];
    return child;
}
// the host's tree: leaves and the levels above them, every level padded with zeros to a multiple of 64
struct PerTree {
    PerShape sh;
    std::vector<float> leaf;
    std::vector<double> node[kPerMaxLevels + 1];       // [1 .. levels]

    explicit PerTree(int64_t C) : sh(per_shape_of(C))
    {
        leaf.assign((size_t)((C + kPerRadix - 1) / kPerRadix) * kPerRadix, 0.0f);
        for (int l = 1; l <= sh.levels; ++l) node[l].assign((size_t)((sh.n[l] + kPerRadix - 1) / kPerRadix) * kPerRadix, 0.0);
    }
    void children(int level, int64_t i, double *v) const                     // of node i at `level` >= 1
    {
        for (int k = 0; k < kPerRadix; ++k)
            v[k] = level == 1 ? (double)leaf[(size_t)i * kPerRadix + k] : node[level - 1][(size_t)i * kPerRadix + k];
    }
    void rebuild_node(int level, int64_t i)
    {
        double c[kPerRadix];
        children(level, i, c);
        per_scan64(c);
        node[level][(size_t)i] = c[kPerRadix - 1];
    }
    void rebuild()
    {
        for (int l = 1; l <= sh.levels; ++l)
            for (int64_t i = 0; i < sh.n[l]; ++i) rebuild_node(l, i);
    }
    void rebuild_path(int64_t slot)
    {
        for (int l = 1; l <= sh.levels; ++l) rebuild_node(l, slot >> (6 * l));
    }
    double total() const { return node[sh.levels][0]; }
    // the slot a descent with m reaches (before the guard against the ring's size)
    int64_t descend(double m) const
    {
        int64_t i = 0;
        for (int l = sh.levels; l >= 1; --l) {
            double v[kPerRadix], c[kPerRadix];
            children(l, i, v);
            for (int k = 0; k < kPerRadix; ++k) c[k] = v[k];
            per_scan64(c);
            i = i * kPerRadix + per_pick(v, c, m);
            if (i >= sh.n[l - 1]) i = sh.n[l - 1] - 1;
        }
        return i;
    }
};

}  // namespace adc
