// adc_sac_norm.h - the law of the running observation and reward normalisers of the soft actor-critic learners.  It is
// adc_td3_norm.h's law on adc_sac.h's learner: the ring outlives the statistics, so the record and the ring hold RAW observations
// and raw rewards, and a batch is normalised when it is sampled.  Only what differs from adc_td3_norm.h is said here.  Shared by the
// device kernels (parts/kernel_norm.inc, the batch kernels of parts/kernel_sac.inc / kernel_sac_pop.inc) and the host twin
// adc_sac_y_norm_host (adc_shims.cpp; the moments' twins are adc_td3_norm_obs_host / adc_td3_norm_rew_host, the law being the same);
// tests/sac_norm_ref.py restates these comments in numpy, bit for bit.
//
//   raw rows   as adc_td3_norm.h: while a SAC normaliser with `observations` lives the record's obs rows and the ring's x / x' are
//              the raw flat observation; the act path still feeds the network (x - shift) * scale.  The store (k_td3_store /
//              k_td3_pop_store as SAC launches them) is handed no vectors, so the x' of the last recorded day is raw too.
//   sampling   every x[j] and x'[j] that enters the actor (the target's and the actor step's), the critics, the target critics or a
//              weight gradient is mlp_normalize(ring[j], shift[j], scale[j]) with the CURRENT vectors of the element's learner
//              (a population: the member's row of the vectors).  The action part t = mlp_tanh(ring.a) is not touched.
//   target     y = sac_y_norm(r, done, q, alpha, lp, law, scale, clip): rs = r * reward_scale; rs = rs * scale (the learner's
//              reward normaliser's current float32 multiplier); with clip > 0: rs = rs < -clip ? -clip : rs; rs = rs > clip ? clip
//              : rs (a NaN passes), exactly td3_y_norm's clip; the rest is sac_y, operation for operation: al = alpha * lp;
//              v = q - al; gv = gamma * v; gvn = gv * nt; y = rs + gvn.  With scale = 1 and clip = 0 these are sac_y's bits (the
//              product with 1.0f is exact).
//   entropy    the entropy term alpha * lp is NOT scaled: only the reward is.  A normalised reward therefore changes what
//              target_entropy and alpha mean relative to the raw reward - the temperature now trades entropy against a return of
//              about unit standard deviation, whatever the env's money scale is - and a multiplier that moves between updates
//              moves that trade with it (no PopArt-style correction of the critics or the temperature is made).
//   moments    the observation moments, the merge, the forgetting, the vectors, the reward scan and its moments are
//              adc_td3_norm.h's unchanged.  The return scan's discount is the SAC learner's gamma (adc_sac_config.gamma; under a
//              population the env's member's, as in force when the update runs); the reward entering the scan is the raw recorded
//              float32, before reward_scale.
//   ordering   collect, store, normaliser update, SAC updates.
#pragma once
#include "adc_sac.h"
#include "adc_td3_norm.h"

namespace adc {

ADC_HD float sac_y_norm_g(float r, int done, float q, float alpha, float lp, float g, const SacLaw &w, float scale, float clip)
{
    const float rs0 = r * w.reward_scale;
    float rs = rs0 * scale;
    if (clip > 0.0f) {
        const float nc = -clip;
        rs = rs < nc ? nc : rs;
        rs = rs > clip ? clip : rs;
    }
    const float nt = done ? 0.0f : 1.0f;
    const float al = alpha * lp, v = q - al, gv = g * v, gvn = gv * nt;
    return rs + gvn;
}
ADC_HD float sac_y_norm(float r, int done, float q, float alpha, float lp, const SacLaw &w, float scale, float clip)
{
    return sac_y_norm_g(r, done, q, alpha, lp, w.gamma, w, scale, clip);
}

}  // namespace adc
