// adc_es.h - the law of the on-device evolution strategy (OpenAI-ES: Salimans et al. 2017) over the MLP policy's parameters:
// counter-addressed antithetic Gaussian noise, centred-rank fitness shaping, the gradient estimate and the Adam / SGD step.
// Shared by the device kernels (parts/kernel_es.inc) and the host twins adc_es_noise_host / adc_es_update_host
// (adc_shims.cpp); tests/es_ref.py restates these comments in numpy, bit for bit.
//
// Every float32 value below is the result of ONE correctly rounded IEEE operation (-ffp-contract=off, correctly rounded float32
// sqrt and division); "f64" marks what is computed in float64.
//
//   flat order the policy network's layers in order, each W[j][h] input-major (index j * n_out + h) followed by its b[h]; P = the
//              length.  (The value network, log_std, the normalisation and the clamps are not parameters of the strategy.)
//   es key     mix64(seed ^ 0x3C6EF372FE94F82B), seed = adc_es_config.seed, or the engine's seed when that is 0 (mix64: adc_mlp.h).
//   noise      eps(i, g)[p] = normal_from_word(word p % 4 of draw(es key, p / 4, ST_ES = 15, pair i, generation g)): never stored,
//              regenerated wherever it is needed.  Nothing else draws from stage 15; the envs' streams do not move.
//   members    M even; members 2i and 2i + 1 are the antithetic pair i: theta_m[p] = theta[p] + (sigma * e), e = eps(i, g)[p] for
//              member 2i and -eps(i, g)[p] for member 2i + 1 (a product, then a sum).
//   fitness    f64: a member's fitness is the sum of its envs' returns, envs ascending, starting from +0, divided by their number;
//              an env's return is the sum of its float64 step rewards over the generation's days, in day order, from +0.
//   shaping    centered_rank: members sorted by (fitness, member index) ascending, a NaN fitness below every number (several
//              NaNs by index); u[m] = rank / (M - 1) - 0.5 in f64 (a division, then a difference).  raw: u[m] = fitness[m].
//   gradient   f64: acc = +0; for pairs i ascending: acc = acc + (u[2i] - u[2i + 1]) * f64(eps(i, g)[p]) (a difference, a product,
//              a sum); g[p] = float32(acc / (f64(M) * f64(sigma))).  The order is by pair, whatever the launch shape.
//   decay      l2 > 0: g[p] = g[p] - (l2 * theta[p]) (a product, then a difference).
//   adam       t = generation + 1; m = (beta1 * m) + ((1 - beta1) * g); v = (beta2 * v) + ((1 - beta2) * (g * g)), with 1 - beta
//              one float32 subtraction; c1 = float32(1 - beta1^t), c2 = float32(1 - beta2^t), beta^t the f64 product of t factors
//              f64(beta) from 1; theta = theta + lr * ((m / c1) / (sqrt(v / c2) + eps))  (ascent; every operation rounded once).
//   sgd        theta = theta + (lr * g).
//   then       generation = generation + 1.
#pragma once
#include "adc_mlp.h"
#include <algorithm>
#include <vector>

namespace adc {

constexpr uint32_t ST_ES = 15;
constexpr int kEsCenteredRank = 0, kEsRaw = 1;
constexpr int kEsAdam = 0, kEsSgd = 1;

ADC_HD uint64_t es_key(uint64_t seed) { return mlp_mix64(seed ^ 0x3C6EF372FE94F82Bull); }

// the four normals of parameters 4q .. 4q + 3 for one pair and generation
ADC_HD void es_noise4(uint64_t key, uint32_t q, uint32_t pair, uint32_t generation, float out[4])
{
    const U4 w = draw(key, q, ST_ES, pair, generation);
    out[0] = normal_from_word(w.x);
    out[1] = normal_from_word(w.y);
    out[2] = normal_from_word(w.z);
    out[3] = normal_from_word(w.w);
}

// member 2i (sign = 0) or 2i + 1 (sign = 1) of pair i
ADC_HD float es_perturbed(float theta, float sigma, float eps, int sign)
{
    const float s = sigma * (sign ? -eps : eps);
    return theta + s;
}

ADC_HD double es_grad_term(double du, float eps) { return du * (double)eps; }
ADC_HD double es_grad_step(double acc, double du, float eps)
{
    const double t = es_grad_term(du, eps);
    return acc + t;
}
ADC_HD float es_grad_finish(double acc, int M, float sigma) { return (float)(acc / ((double)M * (double)sigma)); }

ADC_HD float es_sqrt(float x) { return __builtin_sqrtf(x); }

struct EsStep {
    int optimiser;
    float lr, beta1, beta2, eps, l2;
    float c1, c2;               // float32(1 - beta^t), from the host
};

ADC_HD float es_decay(float g, float theta, float l2)
{
    if (l2 > 0.0f) {
        const float d = l2 * theta;
        g = g - d;
    }
    return g;
}

// one parameter's step: g is the (decayed) gradient estimate; m, v the Adam moments (untouched by SGD)
ADC_HD float es_apply(const EsStep &s, float theta, float g, float &m, float &v)
{
    if (s.optimiser == kEsSgd) {
        const float d = s.lr * g;
        return theta + d;
    }
    const float a1 = s.beta1 * m, o1 = 1.0f - s.beta1, b1 = o1 * g;
    m = a1 + b1;
    const float a2 = s.beta2 * v, o2 = 1.0f - s.beta2, gg = g * g, b2 = o2 * gg;
    v = a2 + b2;
    const float mh = m / s.c1, vh = v / s.c2;
    const float den = es_sqrt(vh) + s.eps;
    const float q = mh / den;
    const float d = s.lr * q;
    return theta + d;
}

// f64 beta^t by t products from 1, then float32(1 - that)
inline float es_bias_correction(float beta, uint32_t t)
{
    double p = 1.0;
    for (uint32_t k = 0; k < t; ++k) p = p * (double)beta;
    return (float)(1.0 - p);
}

// the shaped pair differences du[i] = u[2i] - u[2i + 1] from the members' fitness (host only: M values)
inline void es_shape(int shaping, const double *fitness, int M, std::vector<double> &du)
{
    std::vector<double> u(fitness, fitness + M);
    if (shaping == kEsCenteredRank) {
        std::vector<int> order((size_t)M);
        for (int m = 0; m < M; ++m) order[(size_t)m] = m;
        std::sort(order.begin(), order.end(), [&](int a, int b) {
            const double fa = fitness[a], fb = fitness[b];
            const bool na = fa != fa, nb = fb != fb;
            if (na != nb) return na;                       // a NaN ranks below every number
            if (!na && fa != fb) return fa < fb;
            return a < b;
        });
        for (int r = 0; r < M; ++r) u[(size_t)order[(size_t)r]] = (double)r / (double)(M - 1) - 0.5;
    }
    du.resize((size_t)(M / 2));
    for (int i = 0; i < M / 2; ++i) du[(size_t)i] = u[(size_t)(2 * i)] - u[(size_t)(2 * i + 1)];
}

}  // namespace adc
