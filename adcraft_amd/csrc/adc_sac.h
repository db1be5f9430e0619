// adc_sac.h - the law of soft actor-critic on the device (Haarnoja, Zhou, Abbeel, Levine 2018; the learned temperature of
// Haarnoja et al. 2018b): a tanh-squashed Gaussian actor, twin critics with Polyak targets, and a temperature alpha whose
// logarithm is a parameter, over adc_td3.h's replay ring.  Shared by the device kernels (parts/kernel_sac.inc) and the host
// twins adc_sac_logp_host / adc_sac_target_host / adc_sac_critic_grad_host / adc_sac_actor_grad_host / adc_sac_alpha_step_host
// (adc_shims.cpp); tests/sac_ref.py restates these comments in numpy, bit for bit.
//
// Every float32 value below is the result of ONE correctly rounded IEEE operation (-ffp-contract=off); "f64" marks what is
// computed in float64.  sum8, the layers, mlp_tanh, mlp_exp, mlp_clamp_log_std, mlp_logp_term and mlp_logp_finish are adc_mlp.h's;
// det_log is adc_law.h's; the hidden deltas, csum, the norm clip and pg_apply are adc_pg.h's; td3_batch_index, td3_min,
// td3_polyak and td3_critic_delta are adc_td3.h's.
//
//   actor      the two-headed policy of adc_mlp_config (last width 2A) with clamp_log_std on; a value network is ignored.
//   head       mean[a] = o[a]; raw[a] = o[A + a]; ls = clamp(raw); sd = mlp_exp(ls); u = mean + sd * z (a product, a sum).
//   squash     t = mlp_tanh(u); w = 1 - t * t; c = det_log(w + eps_sq)      (eps_sq: configuration, default 1e-6)
//   log pi     lp = mlp_logp_finish(sum8(A, a -> mlp_logp_term(z, ls)), A) - sum8(A, a -> c[a])
//   critics    two Q networks on [x | t]: the squashed action in [-1, 1] is the critics' action input; no action normalisation.
//              The ring holds u (k_td3_store as it is); the critic pass takes t = mlp_tanh(ring.a).
//   key        td3_key(seed); batch indices: td3_batch_index (stage 16).  z' of the target: stage ST_SAC_NEXT = 20, z of the actor
//              step: ST_SAC_PI = 21, both addressed (a / 4, stage, b, u) as td3_noise is.  No env or agent stream moves.
//   target     (mean', ls') = the LIVE actor on x' (no target actor); u', t', lp' as above with z';
//              q = td3_min(Q1'([x'|t']), Q2'([x'|t'])); al = alpha * lp'; v = q - al; gv = gamma * v; gvn = gv * nt;
//              y = (r * reward_scale) + gvn.  Under n-step returns (adc_td3.h "n-step") r is the slot's R and gv = gn * v.
//   critic     as adc_td3.h's, on [x | t]; one pg_apply step on psi with critic_lr, t = updates + 1.
//   actor      every update, after the critic step, same batch: (mean, ls), z, u, t, w, lp; q_i = Q_i([x | t]) for both UPDATED
//              critics; i* = q_2 < q_1 ? 2 : 1 (a tie takes critic 1); output delta +1 on critic i*, its hidden deltas, one layer
//              further to the action inputs without an activation derivative (adc_td3.h's din): gq[a].
//              k = (t + t) * w; k = k / (w + eps_sq); s1 = alpha * k; s2 = gq * w; du = s1 - s2.
//              dmean[a] = du; dls[a] = (du * (sd * z)) - alpha, or +0 where the clamp moved raw[a] (pg_clamp_moved).
//              These are the policy output layer's deltas (means, then log-stds); backward, gradient, clip, pg_apply with
//              actor_lr (t = updates + 1).  loss piece: (alpha * lp) - q_{i*}.
//   alpha      the parameter is log_alpha (float32), alpha = mlp_exp(log_alpha); it starts as det_log(init_alpha) with zero
//              moments.  alpha_lr > 0: after the actor step,
//              g = float32(-(csum(B, f64(lp_b)) / f64(B) + f64(target_entropy))) from the actor step's lp; one pg_apply on
//              log_alpha (its own m, v; t = updates + 1); alpha follows.  alpha_lr == 0: alpha stays.  The target and the actor
//              step of update u read the alpha that update u began with.
//   targets    (updates + 1) % target_update_interval == 0: td3_polyak on both target critics.  Then updates + 1.
//   statistics f64 csum / B: critic loss, mean Q1, Q2, y, actor loss, mean lp (entropy estimate = its negative), alpha,
//              log_alpha, both gradient norms before the clip.
#pragma once
#include "adc_td3.h"

namespace adc {

constexpr uint32_t ST_SAC_NEXT = 20, ST_SAC_PI = 21;
// a batch element's pieces: adc_td3.h's first five (kTd3Loss1 .. kTd3Y), then the actor's loss piece, lp, and 1 where the element took critic 2
enum { kSacPiLoss = 5, kSacLp = 6, kSacPick = 7 };

struct SacLaw {
    float gamma, tau, reward_scale, eps_sq, ls_lo, ls_hi;
};
template <class MlpConfig, class SacConfig>
inline SacLaw sac_law_of(const MlpConfig &m, const SacConfig &c)
{
    return SacLaw{c.gamma, c.tau, c.reward_scale, c.eps_sq, m.log_std_lo, m.log_std_hi};
}
// the networks' shape: adc_td3.h's, with the actor's last width 2A
template <class MlpConfig, class SacConfig>
inline Td3Shape sac_shape_of(const MlpConfig &m, int K, const SacConfig &c, int frames = 1)
{
    return td3_shape_of(m, K, c, 0, frames);
}

ADC_HD float sac_noise(uint64_t key, uint32_t stage, int a, uint32_t b, uint32_t update)
{
    const U4 w = draw(key, (uint32_t)(a >> 2), stage, b, update);
    return normal_from_word(td3_word(w, a & 3));
}

// one component of the head: everything the target and the actor step need of it
struct SacHead {
    float ls, sd, u, t, w, c, term;     // clamp(raw), exp(ls), the action before the squash, tanh(u), 1 - t^2, the correction, the Gaussian's term
    int moved;                          // the clamp moved raw
};
ADC_HD SacHead sac_head(float mean, float raw, float z, const SacLaw &law)
{
    SacHead h;
    h.moved = pg_clamp_moved(raw, 1, law.ls_lo, law.ls_hi);
    h.ls = mlp_clamp_log_std(raw, 1, law.ls_lo, law.ls_hi);
    h.sd = mlp_exp(h.ls);
    const float p = h.sd * z;
    h.u = mean + p;
    h.t = mlp_tanh(h.u);
    const float tt = h.t * h.t;
    h.w = 1.0f - tt;
    h.c = det_log(h.w + law.eps_sq);
    h.term = mlp_logp_term(z, h.ls);
    return h;
}
ADC_HD float sac_lp_finish(float sum_terms, float sum_c, int A) { return mlp_logp_finish(sum_terms, A) - sum_c; }

// g: the bootstrap discount, the law's gamma or the slot's gn (adc_td3.h "n-step": gv = gn * v)
ADC_HD float sac_y_g(float r, int done, float q, float alpha, float lp, float g, const SacLaw &w)
{
    const float rs = r * w.reward_scale;
    const float nt = done ? 0.0f : 1.0f;
    const float al = alpha * lp, v = q - al, gv = g * v, gvn = gv * nt;
    return rs + gvn;
}
ADC_HD float sac_y(float r, int done, float q, float alpha, float lp, const SacLaw &w) { return sac_y_g(r, done, q, alpha, lp, w.gamma, w); }
// the loss's derivative by u from gq = dQ / dt
ADC_HD float sac_du(float t, float w, float gq, float alpha, float eps_sq)
{
    float k = (t + t) * w;
    k = k / (w + eps_sq);
    const float s1 = alpha * k, s2 = gq * w;
    return s1 - s2;
}
ADC_HD float sac_dls(float du, float sd, float z, float alpha, int moved)
{
    if (moved) return 0.0f;
    const float sz = sd * z, p = du * sz;
    return p - alpha;
}
ADC_HD float sac_pi_loss(float alpha, float lp, float q)
{
    const float al = alpha * lp;
    return al - q;
}
ADC_HD int sac_pick(float q1, float q2) { return q2 < q1 ? 1 : 0; }        // the critic the actor climbs: 0 or 1
ADC_HD float sac_log_alpha_init(float init_alpha) { return det_log(init_alpha); }
// the temperature's gradient from the chunked sum of the actor step's lp
ADC_HD float sac_alpha_grad(double lp_sum, int64_t B, float target_entropy)
{
    const double mean = lp_sum / (double)B, s = mean + (double)target_entropy;
    return (float)(-s);
}
// one step on log_alpha; returns the new log_alpha, alpha follows
ADC_HD float sac_alpha_step(const EsStep &s, float log_alpha, float g, float &m, float &v, float &alpha)
{
    const float la = pg_apply(s, log_alpha, g, m, v);
    alpha = mlp_exp(la);
    return la;
}

// ---- the host's side: the actor's head on a forward's outputs o[2A], with z from the stage's draw ---------------------------------
// heads[A] filled; returns lp
inline float sac_heads_host(const float *o, int A, uint64_t key, uint32_t stage, uint32_t b, uint32_t update, const SacLaw &law, SacHead *heads,
                            const float *z_given)
{
    for (int a = 0; a < A; ++a) heads[a] = sac_head(o[a], o[A + a], z_given ? z_given[a] : sac_noise(key, stage, a, b, update), law);
    const float st = td3_sum8(A, [&](int a) { return heads[a].term; });
    const float sc = td3_sum8(A, [&](int a) { return heads[a].c; });
    return sac_lp_finish(st, sc, A);
}

}  // namespace adc
