// adc_pg.h - the law of policy-gradient training on the device: generalised advantage estimation (Schulman et al. 2016) over
// the rollout record, the forward recompute and the backward pass of the MLP policy and value networks, the PPO-clip loss
// (Schulman et al. 2017; A2C - Mnih et al. 2016 - is its unclipped first epoch), the optional global gradient-norm clip and
// the Adam / SGD descent step.  Shared by the device kernels (parts/kernel_pg.inc) and the host twins adc_pg_gae_host /
// adc_pg_grad_host / adc_pg_step_host (adc_shims.cpp); tests/pg_ref.py restates these comments in numpy, bit for bit.
//
// Every float32 value below is the result of ONE correctly rounded IEEE operation (-ffp-contract=off, correctly rounded float32
// division and sqrt); "f64" marks what is computed in float64.  sum8, tanh, exp, the layers and the log-probability are
// adc_mlp.h's; the Adam arithmetic is adc_es.h's with the sign of the step turned.
//
//   flat order theta[Q]: the policy network's layers in adc_es.h's order (each W[j][h] input-major at j * n_out + h, then its
//              b[h]), then the value network's layers in the same form, then log_std[A] when the head is the free vector.  A
//              two-headed policy has no third part, a policy without a value network no second.  (b[h] sits where a row
//              j = n_in of W would: index n_in * n_out + h; log_std is such a bias row of a layer without inputs.)
//   chunked    csum(n, t): the f64 sum of n f64 terms t(0) .. t(n-1) in chunks of kPgChunk = 1024 consecutive indices: total = +0;
//              for chunks ascending: part = +0; for the chunk's indices ascending: part = part + t(i); then total = total + part.
//              Where t(i) is the f64 product of two float32 values it is exact, so a chain step may be one fused multiply-add
//              (the device) or a product and a sum (the host): the same bits.  Nothing about a launch - workgroups, env
//              groups, where a minibatch begins - enters the order.
//
//   GAE        per env, over the recorded days t = T-1 .. 0, float32: r = reward * reward_scale; done = terminated | truncated;
//              nt = done ? 0 : 1; next = t == T-1 ? bootstrap value : value[t+1]; gl = gamma * lambda (once);
//              delta = (r + ((gamma * next) * nt)) - value[t];  adv[t] = delta + ((gl * nt) * adv[t+1]) (adv[T] = +0);
//              ret[t] = adv[t] + value[t].  A day that ends an episode bootstraps nothing, truncated or terminated: the record
//              holds no value of the observation before the reset (Stable-Baselines3 and RLlib's default do the same).
//   normalise  optional, over ALL recorded samples (index t * N + env) - not per minibatch, so that how an update is cut into
//              minibatches does not enter: mean = csum(f64(adv)) / f64(n); var = csum(d * d, d = f64(adv) - mean; the square
//              rounded, then added) / f64(n) (the population variance); std = f64 sqrt(var) (on the host);
//              adv = float32((f64(adv) - mean) / (std + 1e-8)).  ret is left as it is.
//
//   forward    on the recorded (already normalised) input row x: adc_mlp.h's layers, every layer's activations kept.
//   head       mean[a] = o[a]; raw[a] = o[A + a] (two heads) or log_std[a]; ls = clamp(raw) (adc_mlp.h); sd = exp(ls);
//              z = (action[a] - mean) / sd (a difference, a division); logp = mlp_logp_finish(sum8(A, mlp_logp_term(z, ls)));
//              ratio = exp(logp - logp_old);  entropy = sum8(A, ls) + float32(A) * (0.5 + 0.91893853) (the sum in the
//              parentheses once, a product, a sum).
//   loss       per sample, the update's loss being the mean over its samples:
//              surrogate  s1 = ratio * adv.  eps_clip > 0: lo = 1 - eps_clip, hi = 1 + eps_clip, rc = ratio < lo ? lo :
//                         ratio > hi ? hi : ratio, s2 = rc * adv, policy loss = -(s1 < s2 ? s1 : s2); "clipped" = ratio < lo or
//                         ratio > hi.  eps_clip <= 0: policy loss = -s1, never clipped (the vanilla policy gradient).
//                         dL/dlogp = g = -(adv * ratio) when the sample is not clipped or s1 < s2 (the unclipped side is the
//                         minimum: the ratio moved the way that lowers the objective), else +0: a clipped sample whose clipped
//                         side is the minimum passes nothing.
//              value      dv = V - ret; value loss = 0.5 * (dv * dv); dL/dV = vf_coef * dv.
//              entropy    the loss holds -ent_coef * entropy: dL/dls[a] has the term -ent_coef.
//              dL/dmean[a] = g * (z / sd);   dL/dls[a] = (g * ((z * z) - 1)) - ent_coef - or +0 when the clamp moved raw[a]
//              (raw < lo or raw > hi: the bound is a constant; a raw value exactly on a bound is not moved and passes, as in
//              torch.clamp).  These are the deltas of the policy network's output layer (means, then log-stds) or, the
//              log-stds' with the free vector, the "delta" of log_std's bias row.  The value network's output delta is dL/dV.
//   backward   delta_l[j] = act'(y_l[j]) * sum8(n_out, h -> W_{l+1}[j][h] * delta_{l+1}[h]) for the hidden layers, last to
//              first; tanh' = 1 - (y * y), relu' = y > 0 ? 1 : 0.  The first layer needs no input delta.
//   gradient   of layer l with input x_l (x_0 = x): dW[j][h] = csum(S, s -> f64(x_l,s[j]) * f64(delta_l,s[h])), db[h] =
//              csum(S, s -> f64(delta_l,s[h])) (the row j = n_in with x = 1); g[p] = float32(total / f64(S)).  Within one
//              gradient call over the envs [n0, n0 + B) and T recorded days, sample s = t * B + (env - n0), S = T * B.
//   norm clip  max_grad_norm > 0: sq = csum(Q, p -> f64(g[p]) * f64(g[p])); norm = f64 sqrt(sq) (on the host);
//              scale = float32(min(1, f64(max_grad_norm) / (norm + 1e-6))); g[p] = g[p] * scale (one float32 product, also when
//              scale is 1).
//   step       t = optimiser steps taken + 1.  adam: m, v, c1, c2 as in adc_es.h (bias corrections from the host);
//              theta = theta - lr * ((m / c1) / (sqrt(v / c2) + eps)).  sgd: theta = theta - (lr * g).  Then steps = steps + 1.
//   statistics f64, each csum(S, f64(piece)) / f64(S): policy loss, value loss, entropy, approximate KL (piece: logp_old -
//              logp, one float32 difference), clip fraction (piece: clipped ? 1 : 0).  Explained variance of the value
//              function at collection: e = ret - value_old (float32); with m_x = csum(f64(x)) / S and q_x = csum(f64(x) * f64(x)) / S:
//              1 - (q_e - m_e * m_e) / (q_r - m_r * m_r).  Gradient norm: `norm` above, before the clip.
#pragma once
#include "adc_es.h"
#include <cmath>
#include <cstdint>
#include <vector>

namespace adc {

constexpr int kPgChunk = 1024;
constexpr int kPgMaxTerms = 2 * kMlpMaxLayers + 1;     // the gradient's terms: every layer of both networks, log_std's row
constexpr int kPgPieces = 8;                           // floats of a sample's loss pieces (below)
enum { kPgPolLoss = 0, kPgValLoss = 1, kPgEntropy = 2, kPgKl = 3, kPgClipped = 4, kPgRet = 5, kPgErr = 6 };
constexpr int kPgSums = 10;                            // the seven pieces, ret^2, err^2, g^2

// both networks and the head
struct PgShape {
    int activation, two_heads, clamp;
    float ls_lo, ls_hi;
    int A, D;
    int layers[2];                                     // [0] policy, [1] value (0: none)
    int n_out[2][kMlpMaxLayers];
};
ADC_HD int pg_n_in(const PgShape &s, int net, int l) { return l == 0 ? s.D : s.n_out[net][l - 1]; }
// floats of a sample's kept hidden activations / of its deltas (every layer's, both networks', then the free log_std's A)
ADC_HD int pg_acts_floats(const PgShape &s)
{
    int n = 0;
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l + 1 < s.layers[net]; ++l) n += s.n_out[net][l];
    return n;
}
ADC_HD int pg_deltas_floats(const PgShape &s)
{
    int n = s.two_heads ? 0 : s.A;
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l < s.layers[net]; ++l) n += s.n_out[net][l];
    return n;
}
ADC_HD int pg_param_count(const PgShape &s)
{
    int q = s.two_heads ? 0 : s.A;
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l < s.layers[net]; ++l) q += (pg_n_in(s, net, l) + 1) * s.n_out[net][l];
    return q;
}

// from an adc_mlp_config (include/adcraft_engine.h) for num_keywords keywords; frames: the policy's observation history
// (adc_mlp.h), its input row is that many flat observations wide
template <class MlpConfig>
inline PgShape pg_shape_of(const MlpConfig &c, int K, int frames = 1)
{
    PgShape s{};
    s.A = K + 1; s.D = frames * (5 * K + 2);
    s.activation = c.activation == 0 ? kMlpTanh : kMlpRelu;
    s.clamp = c.clamp_log_std != 0; s.ls_lo = c.log_std_lo; s.ls_hi = c.log_std_hi;
    s.layers[0] = c.n_policy_layers; s.layers[1] = c.n_value_layers;
    for (int l = 0; l < kMlpMaxLayers; ++l) { s.n_out[0][l] = c.policy_widths[l]; s.n_out[1][l] = c.value_widths[l]; }
    s.two_heads = c.policy_widths[c.n_policy_layers - 1] == 2 * s.A;
    return s;
}

struct PgLoss {
    float eps_clip, vf_coef, ent_coef;
};

// ---- GAE, one day of one env ------------------------------------------------------------------------------------------------
ADC_HD float pg_gae_day(float reward, float reward_scale, int done, float value, float next, float gamma, float gl, float &adv_next)
{
    const float r = reward * reward_scale;
    const float nt = done ? 0.0f : 1.0f;
    const float gn = gamma * next, gnn = gn * nt;
    const float d1 = r + gnn, delta = d1 - value;
    const float gln = gl * nt, ga = gln * adv_next;
    adv_next = delta + ga;
    return adv_next;
}
ADC_HD float pg_normalized(float adv, double mean, double std)
{
    const double d = (double)adv - mean, den = std + 1e-8;
    return (float)(d / den);
}

// ---- the head ---------------------------------------------------------------------------------------------------------------
ADC_HD float pg_z(float action, float mean, float sd)
{
    const float d = action - mean;
    return d / sd;
}
ADC_HD float pg_entropy_finish(float sum_ls, int A)
{
    const float c = 0.5f + 0.918938517570495605f;
    const float fa = (float)A * c;
    return sum_ls + fa;
}
// the surrogate of one sample: its policy loss, whether the ratio is clipped, and g = dL/dlogp
ADC_HD float pg_surrogate(float ratio, float adv, float eps_clip, float &pol_loss, int &clipped)
{
    const float s1 = ratio * adv;
    bool pass = true;
    float s = s1;
    clipped = 0;
    if (eps_clip > 0.0f) {
        const float lo = 1.0f - eps_clip, hi = 1.0f + eps_clip;
        const float rc = ratio < lo ? lo : ratio > hi ? hi : ratio;
        const float s2 = rc * adv;
        clipped = ratio < lo || ratio > hi;
        s = s1 < s2 ? s1 : s2;
        pass = !clipped || s1 < s2;
    }
    pol_loss = -s;
    if (!pass) return 0.0f;
    const float ar = adv * ratio;
    return -ar;
}
ADC_HD float pg_dmean(float g, float z, float sd)
{
    const float q = z / sd;
    return g * q;
}
ADC_HD float pg_dls(float g, float z, float ent_coef, int moved)
{
    if (moved) return 0.0f;
    const float zz = z * z, e = zz - 1.0f, p = g * e;
    return p - ent_coef;
}
ADC_HD int pg_clamp_moved(float raw, int clamp, float lo, float hi) { return clamp && (raw < lo || raw > hi); }
ADC_HD float pg_dvalue(float V, float ret, float vf_coef, float &val_loss)
{
    const float dv = V - ret, sq = dv * dv;
    val_loss = 0.5f * sq;
    return vf_coef * dv;
}
// act'(y) * s for a hidden neuron with activation y and the weighted sum s of the next layer's deltas
ADC_HD float pg_hidden_delta(float y, float s, int activation)
{
    float d;
    if (activation == kMlpTanh) {
        const float yy = y * y;
        d = 1.0f - yy;
    } else d = y > 0.0f ? 1.0f : 0.0f;
    return d * s;
}

// ---- sums over samples / parameters -------------------------------------------------------------------------------------------
// one chain step with an exact f64 product (fused on the device, a product and a sum on the host: the same bits)
ADC_HD double pg_chain_mac(double part, float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_fma((double)a, (double)b, part);
#else
    const double p = (double)a * (double)b;
    return part + p;
#endif
}
ADC_HD double pg_chain_sqdev(double part, float a, double mean)
{
    const double d = (double)a - mean, sq = d * d;
    return part + sq;
}
ADC_HD float pg_grad_finish(double total, int64_t count) { return (float)(total / (double)count); }

template <class Term>
inline double pg_csum(int64_t n, Term step)      // step(part, i) -> part advanced by term i
{
    double total = 0.0;
    for (int64_t c0 = 0; c0 < n; c0 += kPgChunk) {
        const int64_t c1 = c0 + kPgChunk < n ? c0 + kPgChunk : n;
        double part = 0.0;
        for (int64_t i = c0; i < c1; ++i) part = step(part, i);
        total = total + part;
    }
    return total;
}

// ---- clip and step ----------------------------------------------------------------------------------------------------------------
// (ADC_HD: k_pg_decide of parts/kernel_pg_queued.inc takes the host's decision on the device - one float64 sum, one float64
//  quotient, one comparison, one rounding to float32: the host's bits)
ADC_HD float pg_clip_scale(float max_grad_norm, double norm)
{
    const double q = (double)max_grad_norm / (norm + 1e-6);
    return (float)(q < 1.0 ? q : 1.0);
}
// es_apply with the sign of the step turned (descent)
ADC_HD float pg_apply(const EsStep &s, float theta, float g, float &m, float &v)
{
    if (s.optimiser == kEsSgd) {
        const float d = s.lr * g;
        return theta - d;
    }
    const float a1 = s.beta1 * m, o1 = 1.0f - s.beta1, b1 = o1 * g;
    m = a1 + b1;
    const float a2 = s.beta2 * v, o2 = 1.0f - s.beta2, gg = g * g, b2 = o2 * gg;
    v = a2 + b2;
    const float mh = m / s.c1, vh = v / s.c2;
    const float den = es_sqrt(vh) + s.eps;
    const float q = mh / den;
    const float d = s.lr * q;
    return theta - d;
}

// the statistics from the ten sums (kPgSums) of an update over S samples
struct PgStatsOut {
    double policy_loss, value_loss, entropy, approx_kl, clip_fraction, grad_norm, explained_variance;
};
// the two statistics a step's decisions need - the target-KL stop and the norm clip - on either side: one float64 division, one
// float64 square root (correctly rounded on the device as on the host: no fast-math)
ADC_HD double pg_stats_approx_kl(const double *sums, int64_t S) { return sums[kPgKl] / (double)S; }
ADC_HD double pg_stats_grad_norm(const double *sums) { return __builtin_sqrt(sums[9]); }
inline PgStatsOut pg_stats_finish(const double *sums, int64_t S)
{
    const double n = (double)S;
    PgStatsOut o;
    o.policy_loss = sums[kPgPolLoss] / n;
    o.value_loss = sums[kPgValLoss] / n;
    o.entropy = sums[kPgEntropy] / n;
    o.approx_kl = pg_stats_approx_kl(sums, S);
    o.clip_fraction = sums[kPgClipped] / n;
    const double mr = sums[kPgRet] / n, me = sums[kPgErr] / n, qr = sums[7] / n, qe = sums[8] / n;
    const double vr = qr - mr * mr, ve = qe - me * me;
    o.explained_variance = 1.0 - ve / vr;
    o.grad_norm = pg_stats_grad_norm(sums);
    return o;
}

// ---- the host's side of a sample: forward, head, loss, backward (the kernel runs the same steps, lanes over neurons) -------------
// theta: flat order.  acts / deltas: pg_acts_floats / pg_deltas_floats values, networks and layers in order (the free log_std's
// A "deltas" last); pieces: kPgPieces floats
// `addon` is PgNoAddon, or adc_pg_kl.h's PgKlSampleHost: the KL penalty and the value-loss clip of one sample, or adc_imitation.h's
// ImSampleHost (Addon::im): the surrogate is the imitation loss's, the pieces at kPgKl / kPgClipped are logp and the weight
struct PgNoAddon {
    static constexpr bool on = false;
    static constexpr bool im = false;
};
template <class Addon>
inline void pg_sample_host_with(const PgShape &sh, const PgLoss &loss, const float *theta, const float *x, const float *action, float logp_old,
                                float adv, float ret, float value_old, float *acts, float *deltas, float *pieces, const Addon &addon)
{
    const int A = sh.A;
    auto sum8 = [](int n, auto term) {
        float s[kMlpChains];
        for (int c = 0; c < kMlpChains; ++c) {
            float acc = 0.0f;
            for (int i = c; i < n; i += kMlpChains) acc = acc + term(i);
            s[c] = acc;
        }
        return mlp_join8(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]);
    };
    // where a network's layers sit in theta, acts and deltas
    const float *W[2][kMlpMaxLayers], *b[2][kMlpMaxLayers];
    float *y[2][kMlpMaxLayers], *dl[2][kMlpMaxLayers];
    std::vector<float> outs[2];
    {
        const float *t = theta;
        float *a = acts, *d = deltas;
        for (int net = 0; net < 2; ++net) {
            outs[net].assign((size_t)(sh.layers[net] ? sh.n_out[net][sh.layers[net] - 1] : 1), 0.0f);
            for (int l = 0; l < sh.layers[net]; ++l) {
                const int n_in = pg_n_in(sh, net, l), n_out = sh.n_out[net][l];
                W[net][l] = t; b[net][l] = t + (size_t)n_in * n_out; t += (size_t)(n_in + 1) * n_out;
                if (l + 1 < sh.layers[net]) { y[net][l] = a; a += n_out; } else y[net][l] = outs[net].data();
                dl[net][l] = d; d += n_out;
            }
        }
    }
    const float *log_std = sh.two_heads ? nullptr : theta + (pg_param_count(sh) - A);
    float *d_free = sh.two_heads ? nullptr : deltas + (pg_deltas_floats(sh) - A);
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l < sh.layers[net]; ++l) {
            const int n_in = pg_n_in(sh, net, l), n_out = sh.n_out[net][l];
            const float *in = l == 0 ? x : y[net][l - 1], *w = W[net][l];
            for (int h = 0; h < n_out; ++h) {
                float s[kMlpChains];
                for (int c = 0; c < kMlpChains; ++c) {
                    float acc = 0.0f;
                    for (int j = c; j < n_in; j += kMlpChains) acc = mlp_mac(acc, w[(size_t)j * n_out + h], in[j]);
                    s[c] = acc;
                }
                const float v = mlp_join8(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]) + b[net][l][h];
                y[net][l][h] = l + 1 < sh.layers[net] ? mlp_act(v, sh.activation) : v;
            }
        }
    // head
    const float *o = outs[0].data();
    std::vector<float> zs((size_t)A), sds((size_t)A), lss((size_t)A);
    std::vector<int> moved((size_t)A);
    for (int a = 0; a < A; ++a) {
        const float raw = sh.two_heads ? o[A + a] : log_std[a];
        const float ls = mlp_clamp_log_std(raw, sh.clamp, sh.ls_lo, sh.ls_hi);
        moved[(size_t)a] = pg_clamp_moved(raw, sh.clamp, sh.ls_lo, sh.ls_hi);
        lss[(size_t)a] = ls;
        sds[(size_t)a] = mlp_exp(ls);
        zs[(size_t)a] = pg_z(action[a], o[a], sds[(size_t)a]);
    }
    const float logp = mlp_logp_finish(sum8(A, [&](int a) { return mlp_logp_term(zs[(size_t)a], lss[(size_t)a]); }), A);
    const float entropy = pg_entropy_finish(sum8(A, [&](int a) { return lss[(size_t)a]; }), A);
    float pol_loss, val_loss, g, w = 0.0f;
    int clipped = 0;
    if constexpr (Addon::im) g = addon.surrogate(adv, logp, pol_loss, w);
    else {
        const float ratio = mlp_exp(logp - logp_old);
        g = pg_surrogate(ratio, adv, loss.eps_clip, pol_loss, clipped);
    }
    const float V = sh.layers[1] ? outs[1][0] : 0.0f;
    float dV;
    if constexpr (Addon::on) dV = addon.value(V, ret, loss.vf_coef, val_loss);
    else dV = pg_dvalue(V, ret, loss.vf_coef, val_loss);
    if constexpr (Addon::on) addon.measure(sum8, A, o, lss.data(), sds.data());
    pieces[kPgPolLoss] = pol_loss; pieces[kPgValLoss] = val_loss; pieces[kPgEntropy] = entropy;
    pieces[kPgKl] = Addon::im ? logp : logp_old - logp;
    pieces[kPgClipped] = Addon::im ? w : clipped ? 1.0f : 0.0f; pieces[kPgRet] = ret; pieces[kPgErr] = ret - value_old; pieces[7] = 0.0f;
    // output deltas
    {
        float *dp = dl[0][sh.layers[0] - 1];
        for (int a = 0; a < A; ++a) {
            dp[a] = pg_dmean(g, zs[(size_t)a], sds[(size_t)a]);
            float d = pg_dls(g, zs[(size_t)a], loss.ent_coef, moved[(size_t)a]);
            if constexpr (Addon::on) addon.penalise(a, o[a], sds[(size_t)a], moved[(size_t)a], dp[a], d);
            if constexpr (Addon::im) d = addon.dls(d);
            if (sh.two_heads) dp[A + a] = d; else d_free[a] = d;
        }
        if (sh.layers[1]) dl[1][sh.layers[1] - 1][0] = dV;
    }
    // hidden deltas, last to first
    for (int net = 0; net < 2; ++net)
        for (int l = sh.layers[net] - 2; l >= 0; --l) {
            const int n = sh.n_out[net][l], n_out = sh.n_out[net][l + 1];
            const float *w = W[net][l + 1], *dn = dl[net][l + 1];
            for (int j = 0; j < n; ++j) {
                const float s = sum8(n_out, [&](int h) { const float p = w[(size_t)j * n_out + h] * dn[h]; return p; });
                dl[net][l][j] = pg_hidden_delta(y[net][l][j], s, sh.activation);
            }
        }
}
inline void pg_sample_host(const PgShape &sh, const PgLoss &loss, const float *theta, const float *x, const float *action, float logp_old,
                           float adv, float ret, float value_old, float *acts, float *deltas, float *pieces)
{
    pg_sample_host_with(sh, loss, theta, x, action, logp_old, adv, ret, value_old, acts, deltas, pieces, PgNoAddon{});
}

}  // namespace adc
