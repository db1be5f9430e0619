// adc_td3_norm.h - the law of the running observation and reward normalisers of the off-policy (TD3) learners.  The replay ring
// outlives the statistics, so nothing in it may depend on them: the rollout record and the ring hold RAW observations and raw
// rewards, and a batch is normalised when it is sampled, with the vectors and the multiplier in force at that moment (what
// Stable-Baselines3's VecNormalize does around a replay buffer).  Shared by the device kernels (parts/kernel_norm.inc, the
// batch kernels of parts/kernel_td3.inc / kernel_td3_pop.inc) and the host twins adc_td3_norm_obs_host / adc_td3_norm_rew_host /
// adc_td3_y_norm_host (adc_shims.cpp); tests/td3_norm_ref.py restates these comments in numpy, bit for bit.
//
// Every float64 value below is the result of ONE correctly rounded IEEE operation (-ffp-contract=off; float64 division and
// square root are correctly rounded on the host and on the device); f64(.) of a float32 and of an int64 below 2^53 is exact.
//
//   raw rows   while a normaliser with `observations` lives the record's obs row of (day, env) is the flat observation the act of
//              that day read (adc_mlp.h mlp_obs_at; zeros on an episode's first day) BEFORE x = (x - shift) * scale; the network
//              itself is still fed the normalised value.  The ring's x and x' are copies of those rows; the x' of the last
//              recorded day is the raw row an act would read now (zeros after an auto-reset).
//   sampling   a batch element's x[j] and x'[j] enter the networks (and the weight gradient) as
//              (ring[j] - shift[j]) * scale[j] (adc_mlp.h mlp_normalize: a difference, a product) with the CURRENT vectors of the
//              element's learner; that is the value the store-time path would have written under the same vectors.
//   target     y = td3_y_norm (adc_td3.h): rs = r * reward_scale; rs = rs * scale (the learner's reward normaliser's current
//              float32 multiplier); with rew_clip > 0: rs = rs < -clip ? -clip : rs; rs = rs > clip ? clip : rs (a NaN passes);
//              y = rs + ((gamma * q) * nt).  With scale = 1 and clip = 0 these are td3_y's bits.
//
//   observation moments, per normaliser (one when shared, one per learner with per_member) and per column j < D:
//     input    x[s][j]: the record's raw rows of the recorded days [t0, T) not yet consumed, sample s = (t - t0) * n + local env,
//              S = (T - t0) * n; n = N for the shared normaliser, n = N / M and local env = env - m n for member m's.
//     sums     sx = csum(S, f64(x)); qx = csum(S, f64(x) * f64(x)): adc_norm.h's chunked sums (kPgChunk = 1024 consecutive
//              samples per chunk, the chunks joined in ascending order).
//     batch    mx = sx / f64(S);  vx = qx / f64(S) - mx * mx (a quotient, a product, a difference);  vx = vx > 0 ? vx : 0 (a NaN
//              becomes 0);  M2b = vx * f64(S).  The rows are raw: (mx, M2b) are raw-space moments, there is no back-conversion.
//     merge    (mx, M2b, S) into (count, mean, M2), and the forgetting under obs_count_cap: adc_norm.h's norm_merge.
//     vectors  var = M2 / f64(count);  sd = sqrt(var);  sd = sd < obs_min_std ? obs_min_std : sd;  shift = f32(mean);
//              scale = f32(1.0 / sd), written in place where the policy kernel and the batch kernels read them.
//              (adc_norm.h norm_finish, raw.)
//
//   reward moments: adc_rew_norm.h's law - the per-env float64 carry G (the env's, not a member's), the scan, the float64
//              chunked moments, rew_norm_finish - with the TD3 learner's gamma as the discount (adc_td3_config.gamma; under a
//              population the env's member's, as in force when the update runs), rew_min_std and rew_count_cap.  The multiplier
//              starts at 1.0f; the reward entering the scan is the raw recorded float32, before reward_scale.
//
//   ordering   collect, store, normaliser update, TD3 updates: the batch is scaled by statistics that include the newest days.
#pragma once
#include "adc_rew_norm.h"
#include "adc_td3.h"
