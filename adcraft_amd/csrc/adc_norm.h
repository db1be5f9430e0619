// adc_norm.h - the law of the running observation normaliser: the mean and the variance of the RAW observation, column by
// column, kept as (count, mean, M2) and merged batch by batch from the rollout record (Chan, Golub, LeVeque 1979: the parallel
// update of the moments; what Stable-Baselines3's VecNormalize and RLlib's MeanStdFilter keep around an env), and the float32
// vectors shift / scale that adc_mlp.h's x = (x - shift) * scale reads.  Shared by the device kernels
// (parts/kernel_norm.inc) and the host twin adc_obs_norm_host (adc_shims.cpp); tests/norm_ref.py restates these comments in
// numpy, bit for bit.
//
// Every float64 value below is the result of ONE correctly rounded IEEE operation (-ffp-contract=off; float64 division and
// square root are correctly rounded on the host and on the device); f64(.) of a float32 and of an int64 below 2^53 is exact.
//
//   input      x[s][j], float32, j < D: the record's network inputs of the recorded days [t0, T) not yet consumed, sample
//              s = (t - t0) * n + local env, S = (T - t0) * n; n = N for the shared normaliser, n = N / M and local env =
//              env - m n for member m's.  The rows are ALREADY normalised by the vectors in force when they were collected (a
//              first-day row is (0 - shift) * scale: a sample like any other).
//   moments    of x, per column, one read of the record: sx = csum(S, f64(x)); qx = csum(S, f64(x) * f64(x)) (the product is
//              exact, so a chain step may be one fused multiply-add: adc_pg.h pg_chain_mac); csum is adc_pg.h's chunked sum
//              (kPgChunk = 1024 consecutive samples per chunk, the chunks joined in ascending order).
//              mx = sx / f64(S);  vx = qx / f64(S) - mx * mx (a quotient, a product, a difference);  vx = vx > 0 ? vx : 0
//              (a NaN becomes 0).
//   raw space  with the column's current float32 shift and scale, sc = f64(scale):  mb = f64(shift) + mx / sc;
//              vb = vx / (sc * sc) (the product first);  M2b = vb * f64(S).
//   merge      into the running (count: int64, mean, M2: f64).  count == 0: mean = mb, M2 = M2b.  Otherwise
//              nt = f64(count) + f64(S);  d = mb - mean;  mean = mean + d * (f64(S) / nt);
//              M2 = (M2 + M2b) + (d * d) * ((f64(count) * f64(S)) / nt).  Then count = count + S.
//   forgetting count_cap > 0 and count > count_cap: M2 = M2 * (f64(count_cap) / f64(count)), then count = count_cap - the
//              horizon a drifting env needs (the mean keeps its value, the next batch weighs more).  count_cap 0: off.
//   vectors    var = M2 / f64(count);  sd = sqrt(var);  sd = sd < min_std ? min_std : sd;  shift = f32(mean);
//              scale = f32(1.0 / sd).  A column that never varies ends at scale = f32(1 / min_std) with x = 0.
#pragma once
#include "adc_pg.h"

namespace adc {

struct NormConfig {
    double min_std;
    int64_t count_cap;
};

// one chain step of sx (qx's is pg_chain_mac(part, x, x))
ADC_HD double norm_chain_sum(double part, float x) { return part + (double)x; }

// the batch's raw-space moments (mb, M2b over S samples) merged into the running (count, mean, M2), then the forgetting: the law's
// "merge" and "forgetting" steps (adc_rew_norm.h's return moments go through the same code)
ADC_HD void norm_merge(const NormConfig &c, double mb, double M2b, int64_t S, int64_t &count, double &mean, double &M2)
{
    const double fs = (double)S;
    if (count == 0) {
        mean = mb;
        M2 = M2b;
    } else {
        const double fc = (double)count;
        const double nt = fc + fs;
        const double d = mb - mean;
        const double w = fs / nt, dw = d * w;
        mean = mean + dw;
        const double m2s = M2 + M2b, dd = d * d, cs = fc * fs, k = cs / nt, t = dd * k;
        M2 = m2s + t;
    }
    count = count + S;
    if (c.count_cap > 0 && count > c.count_cap) {
        const double f = (double)c.count_cap / (double)count;
        M2 = M2 * f;
        count = c.count_cap;
    }
}

// the law's "moments": sx, qx over S samples into the batch's mean and its variance, clamped at 0 (a NaN becomes 0)
ADC_HD void norm_batch_moments(double sx, double qx, int64_t S, double &mx, double &vx)
{
    const double fs = (double)S;
    mx = sx / fs;
    const double qm = qx / fs, mm = mx * mx;
    vx = qm - mm;
    vx = vx > 0.0 ? vx : 0.0;
}

// the law's "raw space": the moments of rows normalised by a column's (shift, scale) taken back through those vectors
ADC_HD void norm_to_raw(float shift, float scale, double &mx, double &vx)
{
    const double sc = (double)scale;
    const double mr = mx / sc;
    mx = (double)shift + mr;
    const double sc2 = sc * sc;
    vx = vx / sc2;
}

// the law's scale: 1 / max(sqrt(M2 / count), min_std), as the float32 the kernels multiply by
ADC_HD float norm_scale(const NormConfig &c, int64_t count, double M2)
{
    const double var = M2 / (double)count;
    double sd = __builtin_sqrt(var);
    sd = sd < c.min_std ? c.min_std : sd;
    return (float)(1.0 / sd);
}

// everything after the chunks are joined, for one column: sx, qx over S samples merged into (count, mean, M2); the new vectors.
// The rows were normalised by (shift, scale), or - raw (adc_td3_norm.h: the TD3 learners' record and ring hold the flat observation
// itself) - the batch's moments are raw-space moments as they stand and there is no back-conversion
ADC_HD void norm_finish(const NormConfig &c, bool raw, double sx, double qx, int64_t S, int64_t &count, double &mean, double &M2, float &shift,
                        float &scale)
{
    double mb, vb;
    norm_batch_moments(sx, qx, S, mb, vb);
    if (!raw) norm_to_raw(shift, scale, mb, vb);
    const double M2b = vb * (double)S;
    norm_merge(c, mb, M2b, S, count, mean, M2);
    shift = (float)mean;
    scale = norm_scale(c, count, M2);
}

}  // namespace adc
