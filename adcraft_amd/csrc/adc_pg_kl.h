// adc_pg_kl.h - the law of the PPO learners' KL penalty and value-loss clip (RLlib's PPO loss: Liang et al. 2018; the adaptive
// coefficient is Schulman et al. 2017, section 4): the analytic KL divergence between the diagonal Gaussian that collected a
// sample and the current one, added to adc_pg.h's loss with a coefficient that adapts to a target after every update, and a cap
// on a sample's squared value error.  Shared by the device kernels (parts/kernel_pg_kl.inc) and the host twins
// adc_pg_kl_grad_host / adc_pg_kl_adapt_host (adc_shims.cpp); tests/pg_kl_ref.py restates these comments in numpy, bit for bit.
//
// As in adc_pg.h every float32 value is the result of ONE correctly rounded IEEE operation (no fused multiply-add), sum8 is
// adc_mlp.h's, csum adc_pg.h's; "f64" marks what is computed in float64.
//
//   old        mean_old[a], ls_old[a]: the policy network's mean output and clamped log-std on the sample's recorded input row
//              under the parameters in force when the snapshot is taken (the start of an update) - adc_pg.h's forward and head on
//              that row, which is bit for bit what the act computed.  Two heads: ls_old is per sample; the free head: one vector
//              [A] (per member under a population), the clamped log_std.  sd_old = exp(ls_old) (adc_mlp.h).
//   KL         per sample, KL(old || new) of the diagonal Gaussians, component a (mean, ls, sd: adc_pg.h's head under theta):
//              v = sd * sd;  v_old = sd_old * sd_old;  dm = mean_old - mean;  dl = ls - ls_old;
//              term[a] = ((dl + ((v_old + (dm * dm)) / (2 * v))) - 0.5)      (2 * v is exact; a division, two sums, a difference)
//              kl = sum8(A, term).  Where nothing has moved term is exactly +0: (0 + (v / (2 v))) - 0.5 = (0 + 0.5) - 0.5.
//   gradient   dKL/dmean[a] = -(dm / v) (a division, a sign);  dKL/dls[a] = 1 - ((v_old + (dm * dm)) / v) - or +0 when the clamp
//              moved raw[a], as adc_pg.h's dL/dls.  With kl_coef != 0 the output deltas of adc_pg.h become
//              dL/dmean[a] = pg_dmean(...) + (kl_coef * dKL/dmean[a]);   dL/dls[a] = pg_dls(...) + (kl_coef * dKL/dls[a])
//              (one product, then one sum).  With kl_coef == 0 nothing is added: the deltas are adc_pg.h's bits (a sum with a
//              zero product could turn a -0 into +0), and the KL is measured all the same.
//   value clip vf_clip > 0: sq = dv * dv (adc_pg.h's dv = V - ret); sq > vf_clip: value loss = 0.5 * vf_clip, dL/dV = +0, the
//              sample counts as value-clipped; else adc_pg.h's value loss and dL/dV.  vf_clip = 0: off, never value-clipped.
//              (adc_pg.h's value loss carries a factor 0.5 that RLlib's does not: RLlib's vf_loss_coeff = 1.0 with
//              vf_clip_param = c is vf_coef = 2.0 with vf_clip = c here - the same capped gradient, half the reported loss.)
//   statistics f64, csum(S, f64(piece)) / f64(S) as adc_pg.h's: the mean KL (piece: kl) and the value-clip fraction (piece:
//              value-clipped ? 1 : 0).
//   adaptation once after an update of all its epochs.  kl = the f64 mean KL of the last epoch: the mean over that epoch's
//              minibatches, in order, of their statistics (as adc_pg_stats is).  f64 comparisons against the float32 target:
//              kl > 2 * f64(kl_target): coef = coef * factor_up;  kl < 0.5 * f64(kl_target): coef = coef * factor_down;  else
//              kept.  One float32 product.  factor_up / factor_down = 0 in the configuration mean 1.5 / 0.5.
#pragma once
#include "adc_pg.h"

namespace adc {

constexpr int kPgKlPieces = 2;                         // floats of a sample's add-on pieces: kl, value-clipped
enum { kPgKlKl = 0, kPgKlVfClipped = 1 };

struct PgKl {
    float coef, vf_clip;
};

ADC_HD float pg_kl_term(float mean, float ls, float sd, float mean_old, float ls_old, float sd_old)
{
    const float v = sd * sd, vo = sd_old * sd_old;
    const float dm = mean_old - mean, dl = ls - ls_old;
    const float dd = dm * dm, num = vo + dd, den = 2.0f * v;
    const float q = num / den, t = dl + q;
    return t - 0.5f;
}
ADC_HD float pg_kl_dmean(float mean, float sd, float mean_old)
{
    const float v = sd * sd, dm = mean_old - mean;
    const float q = dm / v;
    return -q;
}
ADC_HD float pg_kl_dls(float mean, float sd, float mean_old, float sd_old, int moved)
{
    if (moved) return 0.0f;
    const float v = sd * sd, vo = sd_old * sd_old;
    const float dm = mean_old - mean, dd = dm * dm, num = vo + dd;
    const float r = num / v;
    return 1.0f - r;
}
// a delta of adc_pg.h with the penalty's share (coef != 0, checked by the caller)
ADC_HD float pg_kl_add(float delta, float coef, float dkl)
{
    const float p = coef * dkl;
    return delta + p;
}
ADC_HD float pg_kl_dvalue(float V, float ret, float vf_coef, float vf_clip, float &val_loss, int &vf_clipped)
{
    const float dv = V - ret, sq = dv * dv;
    if (vf_clip > 0.0f && sq > vf_clip) {
        val_loss = 0.5f * vf_clip;
        vf_clipped = 1;
        return 0.0f;
    }
    vf_clipped = 0;
    val_loss = 0.5f * sq;
    return vf_coef * dv;
}

struct PgKlAdapt {
    float kl_target, factor_up, factor_down;
    int adaptive;
};
template <class KlConfig>
inline PgKlAdapt pg_kl_adapt_of(const KlConfig &c)
{
    return PgKlAdapt{c.kl_target, c.factor_up == 0.0f ? 1.5f : c.factor_up, c.factor_down == 0.0f ? 0.5f : c.factor_down, c.adaptive != 0};
}
inline float pg_kl_adapt(const PgKlAdapt &a, float coef, double kl)
{
    if (!a.adaptive) return coef;
    const double t = (double)a.kl_target;
    if (kl > 2.0 * t) return coef * a.factor_up;
    if (kl < 0.5 * t) return coef * a.factor_down;
    return coef;
}

// the host's side of a sample: adc_pg.h's pg_sample_host_with under this add-on.  mean_old / ls_old: the sample's rows [A]
// (ls_old the shared vector with the free head); pieces: kPgKlPieces floats
struct PgKlSampleHost {
    static constexpr bool on = true;
    static constexpr bool im = false;
    PgKl kl;
    const float *mean_old, *ls_old;
    float *pieces;
    float value(float V, float ret, float vf_coef, float &val_loss) const
    {
        int clipped;
        const float d = pg_kl_dvalue(V, ret, vf_coef, kl.vf_clip, val_loss, clipped);
        pieces[kPgKlVfClipped] = clipped ? 1.0f : 0.0f;
        return d;
    }
    template <class Sum8>
    void measure(Sum8 sum8, int A, const float *mean, const float *ls, const float *sd) const
    {
        pieces[kPgKlKl] = sum8(A, [&](int a) { return pg_kl_term(mean[a], ls[a], sd[a], mean_old[a], ls_old[a], mlp_exp(ls_old[a])); });
    }
    void penalise(int a, float mean, float sd, int moved, float &dmean, float &dls) const
    {
        if (kl.coef == 0.0f) return;
        dmean = pg_kl_add(dmean, kl.coef, pg_kl_dmean(mean, sd, mean_old[a]));
        dls = pg_kl_add(dls, kl.coef, pg_kl_dls(mean, sd, mean_old[a], mlp_exp(ls_old[a]), moved));
    }
};

}  // namespace adc
