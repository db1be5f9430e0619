// adc_td3.h - the law of off-policy training on the device: TD3 (Fujimoto, van Hoof, Meger 2018: twin critics, clipped target
// smoothing noise, delayed actor and target updates) on top of the deterministic policy gradient (Lillicrap et al. 2016), over
// a device-resident replay ring filled from the rollout record.  Shared by the device kernels (parts/kernel_td3.inc) and the
// host twins adc_td3_batch_indices_host / adc_td3_target_host / adc_td3_critic_grad_host / adc_td3_actor_grad_host /
// adc_td3_polyak_host (adc_shims.cpp); tests/td3_ref.py restates these comments in numpy, bit for bit.  The n-step add-on's twins are
// adc_replay_nstep_host / adc_td3_y_nstep_host / adc_sac_y_nstep_host, its restatement tests/nstep_ref.py.  The bounded law's twins
// are adc_td3_bounded_target_host / adc_td3_bounded_actor_grad_host, its restatement tests/td3_bounded_ref.py.
//
// Every float32 value below is the result of ONE correctly rounded IEEE operation (-ffp-contract=off); "f64" marks what is
// computed in float64.  sum8, the layers, tanh and mix64 are adc_mlp.h's; the hidden deltas, csum, the norm clip and the Adam /
// SGD descent step (pg_apply) are adc_pg.h's.
//
//   actor      the policy network of adc_mlp_config with the free log_std[A] head: A = K+1 means on the D = 5K+2 inputs; its
//              mean is the deterministic action.  Exploration at collection is the stochastic act mean + exp(log_std) * z; TD3
//              never trains log_std, and ignores a value network.
//   critics    two Q networks of 1..4 layers, hidden widths <= kMlpMaxWidth, the last width 1, the policy's activation between
//              layers.  Input row [x | an], D + A floats: x the recorded (already normalised) network input, an[a] =
//              (action[a] - a_shift[a]) * a_scale[a] (a subtraction, a product), or an[a] = action[a] without an action
//              normalisation.
//   targets    a copy of the actor's layers and of both critics, made at init and by td3_sync_targets.
//   flat order theta[P]: the policy layers, each W[j][h] input-major (index j * n_out + h) followed by its b[h] (adc_es.h's order).
//              psi[2 Qc]: critic 1's layers in the same form, then critic 2's.  The targets use the same orders.
//   transition of recorded day t and env n: x = the record's obs row (t, n); a = its unclipped action; r = its float32 reward;
//              done = terminated | truncated; x' = the record's obs row (t + 1, n) when day t + 1 is recorded, else the input row an
//              act would read now (the flat observation, zeros after an auto-reset, normalised).  A day that ends an episode
//              bootstraps nothing, truncated or terminated (adc_pg.h's GAE, for the same reason).
//   ring       capacity C.  store appends the `count` samples s = t * N + n of the recorded days not yet stored at slot
//              (written + s) mod C; a sample with s + C < count would be overwritten by the same store and is not written.
//              Then written = written + count, size = min(written, C).
//   td3 key    mix64(seed ^ 0x6A09E667F3BCC908), seed = adc_td3_config.seed, or the engine's seed when that is 0.
//   batch      update number u (the critic updates taken so far, from 0), element b: idx = (uint64(w) * size) >> 32, w = word b % 4
//              of draw(td3 key, b / 4, ST_TD3_BATCH = 16, 0, u).  Duplicates are plain samples.
//   target     mu' = the target actor's means on x'.  n = normal_from_word(word a % 4 of draw(td3 key, a / 4, ST_TD3_NOISE = 17,
//              b, u)) (b in the keyword field).  e = sigma_t * n; e = e < -c ? -c : e; e = e > c ? c : e (nc = -c once).
//              a' = mu'[a] + e; with action_hi > action_lo: a' = a' < lo ? lo : a'; a' = a' > hi ? hi : a'.
//              q = min(Q1'([x' | an']), Q2'([x' | an'])), min(x, y) = x < y ? x : y.  nt = done ? 0 : 1.
//              y = (r * reward_scale) + ((gamma * q) * nt).
//   n-step     the add-on adc_engine_replay_nstep_init(n), n in 1..16; off: everything above.  The store covers the record's days
//              [t0, t1).  For the sample of recorded day t and env e, with the learner's own gamma:
//                  R = r[t]; g = gamma; m = 1; d = done[t]
//                  while m < n and not d and t + m < t1:
//                      p = g * r[t + m]; R = R + p; g = g * gamma; d = done[t + m]; m = m + 1
//              (a product, a sum, a product per summed day).  The slot's x and a are the transition's; r holds R; done holds d, the
//              last summed day's flag; a per-slot float gn holds g, the bootstrap discount: gamma multiplied m - 1 times by gamma
//              (no powf).  x' = the record's obs row (t + m, e) when t + m < t1, else the input row an act would read now (the
//              transition's rule, history and normalisation included), also when d is set; nt = 0 makes it inert.  A window is cut at
//              the first day that ends an episode and at the end of the stored fragment: the last n - 1 days of every store carry
//              m < n, and their gn says so.  The target reads gn[slot] where it reads gamma: y = (R * reward_scale) + ((gn * q) *
//              nt); the normalisers' multiplier and clip apply to R as they did to r.  With n = 1: R = r, gn = gamma, the ring and
//              y are the add-on-off bits.  Slots, written, size, the skipped samples, the batch, the noise and the priorities do
//              not move.  A slot keeps the R and gn it was stored with when its learner's gamma changes later.
//   critic     per critic i: d = Qi([x | an]) - y; loss piece 0.5 * (d * d); output delta d; hidden deltas as in adc_pg.h.
//              g[p] = float32(csum(B, b -> f64(x_l,b[j]) * f64(delta_l,b[h])) / f64(B)) over the batch elements in order, for all
//              of psi.  max_grad_norm > 0: the global norm clip over psi (adc_pg.h).  One pg_apply step with critic_lr,
//              t = updates + 1.  Then updates = updates + 1.
//   actor      only when (u + 1) % policy_delay == 0, after the critic step, on the same batch: mu = the actor's means on x;
//              critic 1 (the updated one) forward on [x | norm(mu)]; its output delta is +1; its hidden deltas as above; one
//              layer further, without an activation derivative: din[j] = sum8(n_out_0, h -> W_0[j][h] * delta_0[h]) for the
//              action inputs j = D .. D + A - 1 alone.  dmu[a] = -(din[D + a] * a_scale[a]) (a product, a negation), or
//              -din[D + a] without a normalisation.  Backward through the policy layers from dmu; gradient, clip and pg_apply
//              with actor_lr (t = actor steps + 1) on theta; the device's policy layers follow theta.  Then actor steps + 1, and
//              Polyak for the target actor and both target critics: t = t + (tau * (p - t)) (a difference, a product, a sum).
//   statistics f64 csum(B, f64(piece)) / f64(B): critic loss (the sum of the two critics' means), mean Q1, mean Q2, mean y, the
//              actor loss -mean Q1(x, mu(x)) of the last actor step; both gradient norms before the clip.
//   bounded    (adc_engine_td3_set_bounded; needs the bounded act of adc_mlp.h, no action normalisation and no action_lo / action_hi)
//              the ring's action is the act's n in [-1, 1], and the critics' action input is n as stored: no tanh, no normalisation.
//              target: t' = mlp_tanh(mu'[a]); a' = td3_target_action(t', n, law) with lo = -1 and hi = 1 in the law's place (sigma_t
//              and c are in units of the half-range).  actor: t = mlp_tanh(mu[a]); critic 1 on [x | t]; din as above;
//              w = 1 - (t * t) (a product, a difference); dmu[a] = -(din[D + a] * w).  Everything else is as above.
//   Training draws from the td3 key's stages 16 and 17 alone: the envs' and the agents' streams do not move.
#pragma once
#include "adc_pg.h"

namespace adc {

constexpr uint32_t ST_TD3_BATCH = 16, ST_TD3_NOISE = 17;
constexpr int kTd3Pieces = 8;                          // floats of a batch element's pieces (below)
enum { kTd3Loss1 = 0, kTd3Loss2 = 1, kTd3Q1 = 2, kTd3Q2 = 3, kTd3Y = 4, kTd3QPi = 5 };

// one fully connected network: n_in inputs, `layers` Linear layers
struct Td3Net {
    int layers, n_in;
    int n_out[kMlpMaxLayers];
};
ADC_HD int td3_n_in(const Td3Net &n, int l) { return l == 0 ? n.n_in : n.n_out[l - 1]; }
ADC_HD int td3_params(const Td3Net &n)
{
    int q = 0;
    for (int l = 0; l < n.layers; ++l) q += (td3_n_in(n, l) + 1) * n.n_out[l];
    return q;
}
ADC_HD int td3_outs(const Td3Net &n)                   // floats of every layer's outputs (= of its deltas)
{
    int q = 0;
    for (int l = 0; l < n.layers; ++l) q += n.n_out[l];
    return q;
}
ADC_HD int td3_hidden(const Td3Net &n) { return td3_outs(n) - n.n_out[n.layers - 1]; }

struct Td3Shape {
    int activation, A, D, norm;                        // norm: an action normalisation was uploaded
    Td3Net pol, q;                                     // the actor (D inputs, A outputs); one critic (D + A inputs, 1 output)
};
ADC_HD int td3_max_width(const Td3Shape &s)
{
    int w = s.A;
    for (int l = 0; l < s.pol.layers; ++l) w = s.pol.n_out[l] > w ? s.pol.n_out[l] : w;
    for (int l = 0; l < s.q.layers; ++l) w = s.q.n_out[l] > w ? s.q.n_out[l] : w;
    return w;
}

struct Td3Law {
    float gamma, tau, noise, noise_clip, lo, hi, reward_scale;
};

// from an adc_mlp_config and an adc_td3_config (include/adcraft_engine.h) for num_keywords keywords; frames: the policy's
// observation history (adc_mlp.h), its input row is that many flat observations wide
template <class MlpConfig, class Td3Config>
inline Td3Shape td3_shape_of(const MlpConfig &m, int K, const Td3Config &c, int norm, int frames = 1)
{
    Td3Shape s{};
    s.A = K + 1; s.D = frames * (5 * K + 2); s.norm = norm;
    s.activation = m.activation == 0 ? kMlpTanh : kMlpRelu;
    s.pol.layers = m.n_policy_layers; s.pol.n_in = s.D;
    s.q.layers = c.n_critic_layers; s.q.n_in = s.D + s.A;
    for (int l = 0; l < kMlpMaxLayers; ++l) { s.pol.n_out[l] = m.policy_widths[l]; s.q.n_out[l] = c.critic_widths[l]; }
    return s;
}
template <class Td3Config>
inline Td3Law td3_law_of(const Td3Config &c)
{
    return Td3Law{c.gamma, c.tau, c.target_noise, c.target_noise_clip, c.action_lo, c.action_hi, c.reward_scale};
}

ADC_HD uint64_t td3_key(uint64_t seed) { return mlp_mix64(seed ^ 0x6A09E667F3BCC908ull); }
ADC_HD uint32_t td3_word(const U4 &w, int h) { return h == 0 ? w.x : h == 1 ? w.y : h == 2 ? w.z : w.w; }

ADC_HD uint32_t td3_batch_index(uint64_t key, uint32_t b, uint32_t update, uint32_t size)
{
    const U4 w = draw(key, b >> 2, ST_TD3_BATCH, 0u, update);
    return (uint32_t)(((uint64_t)td3_word(w, (int)(b & 3u)) * (uint64_t)size) >> 32);
}
ADC_HD float td3_noise(uint64_t key, int a, uint32_t b, uint32_t update)
{
    const U4 w = draw(key, (uint32_t)(a >> 2), ST_TD3_NOISE, b, update);
    return normal_from_word(td3_word(w, a & 3));
}
ADC_HD float td3_action_norm(float a, const float *shift, const float *scale, int i, int norm)
{
    return norm ? mlp_normalize(a, shift[i], scale[i]) : a;
}
ADC_HD float td3_target_action(float mu, float n, const Td3Law &w)
{
    const float nc = -w.noise_clip;
    float e = w.noise * n;
    e = e < nc ? nc : e;
    e = e > w.noise_clip ? w.noise_clip : e;
    float a = mu + e;
    if (w.hi > w.lo) {
        a = a < w.lo ? w.lo : a;
        a = a > w.hi ? w.hi : a;
    }
    return a;
}
ADC_HD float td3_min(float x, float y) { return x < y ? x : y; }
// g: the bootstrap discount, the law's gamma or the slot's gn (n-step)
ADC_HD float td3_y_g(float r, int done, float q, float g, const Td3Law &w)
{
    const float rs = r * w.reward_scale;
    const float nt = done ? 0.0f : 1.0f;
    const float gq = g * q, gqn = gq * nt;
    return rs + gqn;
}
ADC_HD float td3_y(float r, int done, float q, const Td3Law &w) { return td3_y_g(r, done, q, w.gamma, w); }
// td3_y under a running reward normaliser (adc_td3_norm.h): rs = r * reward_scale; rs = rs * scale (the learner's normaliser's
// current multiplier); with clip > 0: rs = rs < -clip ? -clip : rs; rs = rs > clip ? clip : rs (a NaN passes).  The rest is
// td3_y, operation for operation; with scale = 1 and clip = 0 these are td3_y's bits (the product with 1.0f is exact).
ADC_HD float td3_y_norm_g(float r, int done, float q, float g, const Td3Law &w, float scale, float clip)
{
    const float rs0 = r * w.reward_scale;
    float rs = rs0 * scale;
    if (clip > 0.0f) {
        const float nc = -clip;
        rs = rs < nc ? nc : rs;
        rs = rs > clip ? clip : rs;
    }
    const float nt = done ? 0.0f : 1.0f;
    const float gq = g * q, gqn = gq * nt;
    return rs + gqn;
}
ADC_HD float td3_y_norm(float r, int done, float q, const Td3Law &w, float scale, float clip)
{
    return td3_y_norm_g(r, done, q, w.gamma, w, scale, clip);
}
// the n-step window of the sample whose first day's words are at reward / term / trunc (one env: a day is `stride` words further),
// `left` = t1 - t recorded days from there, left >= 1: R, the bootstrap discount g, the last summed day's flag, m
constexpr int kNstepMax = 16;
struct Td3Window {
    float R, g;
    int done, m;
};
ADC_HD Td3Window td3_nstep_window(const float *reward, const uint8_t *term, const uint8_t *trunc, size_t stride, int left, int n, float gamma)
{
    Td3Window w;
    w.R = reward[0]; w.g = gamma; w.m = 1;
    w.done = (term[0] | trunc[0]) ? 1 : 0;
    while (w.m < n && !w.done && w.m < left) {
        const size_t i = (size_t)w.m * stride;
        const float p = w.g * reward[i];
        w.R = w.R + p;
        w.g = w.g * gamma;
        w.done = (term[i] | trunc[i]) ? 1 : 0;
        w.m = w.m + 1;
    }
    return w;
}
ADC_HD float td3_critic_delta(float q, float y, float &loss)
{
    const float d = q - y, sq = d * d;
    loss = 0.5f * sq;
    return d;
}
ADC_HD float td3_dmu(float din, float scale, int norm)
{
    if (!norm) return -din;
    const float p = din * scale;
    return -p;
}
// ... of the bounded actor: through t = tanh(mu)
ADC_HD float td3_dmu_bounded(float din, float t)
{
    const float tt = t * t, w = 1.0f - tt, p = din * w;
    return -p;
}
// the law a bounded learner's target action is formed under: the box is [-1, 1]
ADC_HD Td3Law td3_law_bounded(Td3Law w)
{
    w.lo = -1.0f; w.hi = 1.0f;
    return w;
}
ADC_HD float td3_polyak(float t, float p, float tau)
{
    const float d = p - t, s = tau * d;
    return t + s;
}

// ---- the host's side of a network: forward with every layer's outputs kept, the hidden deltas, the input deltas -------------------
// flat: the network's layers in the flat order.  ys / deltas: td3_outs floats, layers in order
template <class Term>
inline float td3_sum8(int n, Term term)
{
    float s[kMlpChains];
    for (int c = 0; c < kMlpChains; ++c) {
        float acc = 0.0f;
        for (int i = c; i < n; i += kMlpChains) acc = acc + term(i);
        s[c] = acc;
    }
    return mlp_join8(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]);
}
inline void td3_forward_host(const Td3Net &net, int activation, const float *flat, const float *in, float *ys)
{
    const float *w = flat;
    float *y = ys;
    for (int l = 0; l < net.layers; ++l) {
        const int n_in = td3_n_in(net, l), n_out = net.n_out[l];
        const float *b = w + (size_t)n_in * n_out;
        for (int h = 0; h < n_out; ++h) {
            const float v = td3_sum8(n_in, [&](int j) { const float p = w[(size_t)j * n_out + h] * in[j]; return p; }) + b[h];
            y[h] = l + 1 < net.layers ? mlp_act(v, activation) : v;
        }
        in = y; y += n_out; w += (size_t)(n_in + 1) * n_out;
    }
}
// the last layer's deltas are given; the hidden layers' are filled, last to first
inline void td3_backward_host(const Td3Net &net, int activation, const float *flat, const float *ys, float *deltas)
{
    const float *W[kMlpMaxLayers];
    int off[kMlpMaxLayers];
    {
        const float *w = flat;
        int o = 0;
        for (int l = 0; l < net.layers; ++l) { W[l] = w; off[l] = o; w += (size_t)(td3_n_in(net, l) + 1) * net.n_out[l]; o += net.n_out[l]; }
    }
    for (int l = net.layers - 2; l >= 0; --l) {
        const int n = net.n_out[l], n_out = net.n_out[l + 1];
        const float *w = W[l + 1], *dn = deltas + off[l + 1];
        for (int j = 0; j < n; ++j) {
            const float s = td3_sum8(n_out, [&](int h) { const float p = w[(size_t)j * n_out + h] * dn[h]; return p; });
            deltas[off[l] + j] = pg_hidden_delta(ys[off[l] + j], s, activation);
        }
    }
}
// din[i] = sum8(n_out_0, h -> W_0[j0 + i][h] * delta_0[h]), i < n: the first layer's deltas carried to inputs j0 .. j0 + n - 1
inline void td3_input_delta_host(const Td3Net &net, const float *flat, const float *deltas, int j0, int n, float *din)
{
    const int n_out = net.n_out[0];
    for (int i = 0; i < n; ++i)
        din[i] = td3_sum8(n_out, [&](int h) { const float p = flat[(size_t)(j0 + i) * n_out + h] * deltas[h]; return p; });
}

}  // namespace adc
