// adc_rew_norm.h - the law of the running reward normaliser: the variance of the DISCOUNTED RETURN, kept as (count, mean, M2) and
// merged batch by batch from the rollout record's rewards (what Stable-Baselines3's VecNormalize(norm_reward=True) keeps around an
// env: the reward is divided by the running standard deviation of the discounted return, never centred), and the float32
// multiplier `scale` that the GAE kernels read.  Shared by the device kernels (parts/kernel_norm.inc) and the host twins
// adc_rew_norm_host / adc_pg_gae_norm_host (adc_shims.cpp); tests/rew_norm_ref.py restates these comments in numpy, bit for bit.
//
// Every float64 value below is the result of ONE correctly rounded IEEE operation (-ffp-contract=off; float64 division and
// square root are correctly rounded on the host and on the device); f64(.) of a float32 and of an int64 below 2^53 is exact.
//
//   state      per normaliser: count (int64), mean, M2 (f64), scale (float32: the reward multiplier); one normaliser when shared,
//              M with per-member normalisers.  Per ENV a carry G[n] (f64): the running discounted return.  It is the env's, not a
//              member's.  At init: count = 0, mean = 0, M2 = 0, scale = 1.0f, G = +0.
//   discount   gamma is the learner's own, the value GAE uses (adc_pg_config.gamma; under a population the env's member's, as in
//              force when the update runs).
//   scan       per env, over the recorded days [t0, T) not yet consumed, ascending:  G = f64(gamma) * G (a product);
//              G = G + f64(reward[t][n]) (a sum);  the sample g[s] = G;  if day t ended the episode (terminated | truncated):
//              G = +0.  The reward is the raw recorded float32, before reward_scale.  Sample s = (t - t0) * n + local env,
//              S = (T - t0) * n; n = N for the shared normaliser, n = N / M and local env = env - m n for member m's.
//   moments    sx = csum(S, g);  qx = csum(S, g * g) (g is f64: the square is rounded, then added); csum is adc_pg.h's chunked sum
//              (kPgChunk = 1024 consecutive samples per chunk, the chunks joined in ascending order).
//              mb = sx / f64(S);  vb = qx / f64(S) - mb * mb (a quotient, a product, a difference);  vb = vb > 0 ? vb : 0 (a NaN
//              becomes 0);  M2b = vb * f64(S).
//   merge      (mb, M2b, S) into (count, mean, M2), and the forgetting under count_cap: adc_norm.h's, the same code (norm_merge).
//   multiplier sd = sqrt(M2 / f64(count));  sd = sd < min_std ? min_std : sd;  scale = f32(1.0 / sd).  The mean only serves the
//              variance: rewards are not centred.  Rewards that are all zero end at scale = f32(1 / min_std).
//
//   GAE under a normaliser, per day of an env:  r = reward * reward_scale (as adc_pg.h);  r = r * scale (the env's normaliser's
//              current multiplier);  with clip > 0: r = r < -clip ? -clip : r;  r = r > clip ? clip : r (a NaN passes).  Everything
//              after that is adc_pg.h's pg_gae_day with r in the place of its reward * reward_scale, operation for operation.
//              With scale = 1 and clip = 0 these are adc_pg.h's bits.
#pragma once
#include "adc_norm.h"

namespace adc {

// one day of one env's scan: the carry advanced, the sample returned
ADC_HD double rew_norm_scan_day(double &G, float gamma, float reward, int done)
{
    const double gg = (double)gamma * G;
    const double g = gg + (double)reward;
    G = done ? 0.0 : g;
    return g;
}

// one chain step of sx and of qx
ADC_HD double rew_norm_chain_sum(double part, double g) { return part + g; }
ADC_HD double rew_norm_chain_sq(double part, double g)
{
    const double sq = g * g;
    return part + sq;
}

// everything after the chunks are joined: sx, qx over S samples merged into (count, mean, M2); the new multiplier
ADC_HD void rew_norm_finish(const NormConfig &c, double sx, double qx, int64_t S, int64_t &count, double &mean, double &M2, float &scale)
{
    double mb, vb;
    norm_batch_moments(sx, qx, S, mb, vb);
    const double M2b = vb * (double)S;
    norm_merge(c, mb, M2b, S, count, mean, M2);
    scale = norm_scale(c, count, M2);
}

// GAE, one day of one env under a normaliser's multiplier and clip (pg_gae_day's product with 1.0f is exact)
ADC_HD float rew_norm_gae_day(float reward, float reward_scale, float scale, float clip, int done, float value, float next, float gamma, float gl,
                              float &adv_next)
{
    const float r0 = reward * reward_scale;
    float r = r0 * scale;
    if (clip > 0.0f) {
        r = r < -clip ? -clip : r;
        r = r > clip ? clip : r;
    }
    return pg_gae_day(r, 1.0f, done, value, next, gamma, gl, adv_next);
}

}  // namespace adc
