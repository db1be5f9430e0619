// adc_imitation.h - the law of imitation learning on the device: behaviour cloning and MARWIL (Wang et al. 2018, "Exponentially
// weighted imitation learning for batched historical data") over a record of teacher days - days on which an expert acted and the
// record kept the network input the learner would have seen next to the expert's action.  Shared by the device kernel
// (parts/kernel_imitation.inc) and the host twins adc_im_weight_host / adc_im_grad_host (adc_shims.cpp); tests/im_ref.py restates
// these comments in numpy, bit for bit.
//
// Every float32 value below is the result of ONE correctly rounded IEEE operation; "f64" marks what is computed in float64.  The
// forward pass, the head, the backward pass, the chunked sums csum, the gradient, the norm clip and the step are adc_pg.h's as they
// are; what is said here replaces that law's "loss" and "statistics" paragraphs.
//
//   returns    adc_pg.h's GAE with lambda = 1 under the trainer's gamma and reward_scale (gl = gamma * 1, a float32 product):
//              ret[t] is the discounted return of the teacher's rewards, cut at episode ends and bootstrapped with V at the record's
//              end; adv = ret - value in GAE's own arithmetic (ret[t] = adv[t] + value[t]).  No advantage normalisation.
//   scale      ma is f64 state and starts at ma_start.  Once per advantages call, over ALL n recorded samples (index t * N + env) -
//              not per minibatch, so that how an update is cut does not enter:  msq = csum(f64(adv) * f64(adv)) / f64(n) (the
//              products exact);  ma = ma + (ma_rate * (msq - ma)) (f64: a difference, a product, a sum);
//              c = float32(1e-8 + f64 sqrt(ma)) (a square root, a sum, one rounding to float32; on the host).
//   weight     beta == 0: w = 1 and no exp is evaluated (behaviour cloning).  Otherwise q = adv / c; e = beta * q; w = exp(e)
//              (adc_mlp.h's exp); then w = w > w_max ? w_max : w when w_max > 0 (a NaN passes).
//   head       adc_pg.h's on the recorded teacher action: z, sd, ls, logp, entropy.
//   loss       per sample, the update's loss being the mean over its samples:
//              policy     wl = w * logp; policy loss = -wl.  dL/dlogp = g = -w.
//                         dL/dmean[a] = pg_dmean(g, z, sd);  dL/dls[a] = pg_dls(g, z, +0, moved) - or +0 for every component when
//                         train_log_std == 0: the free log_std then is not trained (it stays what the user set: with log_std = 0
//                         the policy loss is a plain squared error of the means, and a per-component log_std is the user's scale
//                         of the action's components).
//              value      pg_dvalue(V, ret, vf_coef) with the imitation configuration's own vf_coef (0 drops it, as RLlib's BC does).
//              no entropy term.
//   pieces     per sample [policy loss, value loss, entropy, logp, w, ret, ret - value, 0]: adc_pg.h's layout with logp where
//              the approximate KL's piece is and w where the clip flag is, summed by the same kernels.
//   statistics f64, each csum(S, f64(piece)) / f64(S): policy loss, value loss, entropy, logp, weight; the explained variance and
//              the gradient norm as in adc_pg.h.
#pragma once
#include "adc_pg.h"

namespace adc {

// what a sample's loss reads beyond PgLoss (vf_coef, and +0 for ent_coef): c is the call's scale, formed on the host
struct ImLaw {
    float beta, c, w_max;
    int train_log_std;
};

// the moving scale's update from the sum of squares over n samples; returns the new ma, c through c_out
inline double im_ma_next(double ma, double ma_rate, double sumsq, int64_t n, float &c_out)
{
    const double msq = sumsq / (double)n;
    const double d = msq - ma, p = ma_rate * d;
    const double next = ma + p;
    const double r = __builtin_sqrt(next), cs = 1e-8 + r;
    c_out = (float)cs;
    return next;
}

ADC_HD float im_weight(float adv, const ImLaw &law)
{
    if (law.beta == 0.0f) return 1.0f;
    const float q = adv / law.c, e = law.beta * q;
    float w = mlp_exp(e);
    if (law.w_max > 0.0f) w = w > law.w_max ? law.w_max : w;
    return w;
}
// the policy loss of one sample and g = dL/dlogp
ADC_HD float im_surrogate(float w, float logp, float &pol_loss)
{
    const float wl = w * logp;
    pol_loss = -wl;
    return -w;
}

// pg_sample_host_with's add-on of an imitation sample (adc_pg.h: Addon::im)
struct ImSampleHost {
    static constexpr bool on = false;
    static constexpr bool im = true;
    ImLaw law;
    float surrogate(float adv, float logp, float &pol_loss, float &w) const
    {
        w = im_weight(adv, law);
        return im_surrogate(w, logp, pol_loss);
    }
    float dls(float d) const { return law.train_log_std ? d : 0.0f; }
};

}  // namespace adc
