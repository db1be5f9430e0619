// adc_mlp.h - the law of the device-resident MLP policy: a fully connected policy network (and an optional value network) on
// the flat observation, a diagonal Gaussian head, and the conversion of the sampled action into the env's cent bids.  Shared
// by the device kernel (parts/kernel_mlp_policy.inc) and the host twin adc_mlp_act_host (adc_shims.cpp), so that CPU tests
// run the very operations the GPU runs; tests/mlp_ref.py restates these comments in numpy, bit for bit (the bounded act:
// adc_mlp_bounded_host / adc_mlp_unbox_host and tests/td3_bounded_ref.py).
//
// Every float32 value below is the result of ONE correctly rounded IEEE operation (build with -ffp-contract=off: no fused
// multiply-add is meant anywhere in this file); "f64" marks the few places that compute in float64 and round once.
//
//   input      x[j], j < D = 5K+2: the flat observation (buyside_clicks[K] | cost[K] | cumulative_profit | days_passed |
//              impressions[K] | revenue[K] | sellside_conversions[K]) as float32; all zeros on the first day of an episode.
//              With normalisation: x[j] = (x[j] - shift[j]) * scale[j] (a subtraction, then a product).
//   sum8(n, t) the sum of n float32 terms t(0) .. t(n-1): eight chains, chain c = ((0 + t(c)) + t(c+8)) + t(c+16) + ... over
//              the j = c (mod 8) in ascending order, starting from +0; then ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)).
//   layer      y[h] = act(sum8(n_in, j -> W[j][h] * x[j]) + b[h]); act = tanh or relu between layers, none after the last.
//              relu(v) = v > 0 ? v : +0 (a NaN becomes +0).
//   exp64(x)   f64, |x| <= 700: n = rint(x * 1.4426950408889634); r = (x - n * 0.693145751953125) - n * 1.4286068203094173e-06;
//              q = c14; q = q * r + c13; ... ; q = q * r + c2 (c_k = 1.0 / k!, k! exact); p = r + (r * r) * q; result
//              (1 + p) * 2^n.  p alone is exp(r) - 1 ("expm1 polynomial").
//   tanh(x)    float32 -> float32, odd: a = |x| as f64; a >= 10: 1; 2a < 0.34: m = expm1 polynomial of r = 2a, t = m / (m + 2);
//              otherwise e = exp64(2a), t = 1 - 2 / (e + 1); result = float32(t) with x's sign.  NaN -> NaN.
//   exp(x)     float32 -> float32: float32(exp64(min(max(x, -87), 88))).  NaN -> NaN.
//   head       the policy network's output o[]: A = K+1 means (then log_std[a] is a free parameter vector) or 2A values, means
//              then log-stds.  Optional clamp: ls = ls < lo ? lo : ls; ls = ls > hi ? hi : ls.
//   agent key  mix64(seed ^ 0x1F83D9ABFB41BD6B) from a per-env seed, or mix64(engine seed ^ mix64(global env id + 0x5BE0CD19137E2179))
//              without one; mix64 = splitmix64: x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;
//              x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31 (64-bit wrap-around).  The tick starts at 0; every act adds 1.
//   sample     z[a] = normal_from_word(word a % 4 of draw(agent key, a / 4, ST_MLP, 0, agent tick)), or handed in (replay), or
//              0 (deterministic).  action a[a] = mean + exp(ls) * z (a product, then a sum); deterministic: a = mean.
//   log-prob   sum8(A, a -> (-((z * z) * 0.5)) - ls[a]) - float32(A) * 0.91893853 (= float32(log(2 pi) / 2)).
//   value      the value network's single output on the same (normalised) input; +0 without one.
//   to the env flat action order [budget, bids...]: bid k from v = a[1 + k]: v > 0.01 ? v : 0.01 (NaN -> 0.01); with an upper clip
//              hi > 0: v < hi ? v : hi; then cents c = rint(f64(v) * 100) clamped to [1, 1e9], bid = float32(c / 100).
//              budget = a[0] > 0.01 ? a[0] : 0.01, or budget_override when that is > 0.
//   squash     (adc_engine_mlp_set_squash; off by default) the env is given e[a] in place of a[a]: t = tanh(a[a]);
//              e[a] = lo[a] + half[a] * (t + 1) (a sum, a product, a sum), half[a] = 0.5 * (hi[a] - lo[a]) formed once on the
//              host.  The bid and the budget are taken from e as above.  The recorded action, the last act's action and the
//              log-probability stay those of the unsquashed a; a deterministic act squashes the mean.
//   bounded    (adc_engine_mlp_set_bounds; off by default; lo[a] < hi[a] finite, half[a] as for the squash) the deterministic actor
//              squashed into the action box, TD3's act.  The action n[a] is in units of the box, in [-1, 1]:
//                  t = tanh(mean[a])
//                  explore (gaussian):  p = exp(ls[a]) * z; n = t + p; n = n < -1 ? -1 : n; n = n > 1 ? 1 : n    (z: the act's own draw)
//                  deterministic:       n = t                                      (wins over either exploration mode)
//                  explore (random):    u = unit_half24(w) of the very word w that z would have been made from (u = (k + 0.5) 2^-24,
//                                       k = w >> 9); v = u + u; n = (v + v) - 1: exact, uniform on the 2^23 points (4k + 2) 2^-24 - 1,
//                                       strictly inside (-1, 1); handed-in normals are not read.  The tick moves as for any act.
//              The env is given e[a] = lo[a] + half[a] * (n + 1): the squash's three operations after its tanh (mlp_box); the bid
//              and the budget are taken from e as above.  The recorded action and the last act's action are n; mean stays the raw
//              mean; logp = +0; value as above.  A deterministic bounded act gives the env the bits the squash gives it.
//              A teacher's action e (the float32 in the action buffers) is recorded as q = (e - lo[a]) * inv_half[a]; n = q - 1;
//              n = n < -1 ? -1 : n; n = n > 1 ? 1 : n, inv_half[a] = 1 / half[a] formed once on the host (mlp_unbox).
//
// Observation history (adc_engine_mlp_init_frames, frames = H in 1..8; H = 1 is everything above, untouched).  D0 = 5K+2.
//   row        D = H * D0; x[f * D0 + j], f < H, j < D0.  Frame 0 is the input above (mlp_obs_at, or zeros when the env's episode
//              day d is 0).  Frame f >= 1 is the raw frame 0 that the act on episode day d - f read if that frame is valid, else
//              zeros.
//   history    hist[N][H][D0], raw float32 (before normalisation).  The act on day d writes its raw frame 0 to slot d mod H after
//              every read of the workgroup (a barrier; frames 1 .. H-1 read the slots (d - f) mod H, never that one).  A second
//              act on the same day (replayed normals) writes the same bits.
//   validity   two words per env: last (the episode day of the last act; -2: none) and from.  At an act on day d:
//              d == 0: from = 0; else if last is neither d - 1 nor d: from = d.  Frame f is valid iff d - f >= from.  Then
//              last = d.  So an auto-reset clears the history through day 0, and days stepped without the agent restart it;
//              an explicit adc_engine_reset sets last = -2 for the envs it resets.  One case is not detected: an auto-reset
//              followed by exactly last + 1 days without an act reads the old episode's frames as the new one's.
//   peek       adc_engine_mlp_bootstrap_value and the x' of a trainer's last stored day evaluate the same rule for "the row an
//              act would read now" and write nothing: not hist, not last, not from.
//   normalise  per position over the whole row: x[i] = (x[i] - shift[i]) * scale[i], i < D, zero frames included (as the first
//              day's zeros are).  The record's obs row is all D of it, normalised or raw as above.
#pragma once
#include "adc_law.h"

namespace adc {

constexpr int kMlpMaxLayers = 4;
constexpr int kMlpMaxTerms = kMlpMaxLayers + 2;    // the (W, b) pairs of a policy's flat order: its layers, and a recurrent policy's Wi and Wh (adc_gru.h)
constexpr int kMlpMaxWidth = 256;          // widest hidden layer; the output layer may be as wide as 2 (K + 1)
constexpr int kMlpChains = 8;
constexpr int kMlpTanh = 0, kMlpRelu = 1;

// one step of a chain: acc + w * x, two roundings
ADC_HD float mlp_mac(float acc, float w, float x)
{
    const float p = w * x;
    return acc + p;
}
// the join of the eight chains (float addition commutes, so a butterfly over lanes c ^ 1, c ^ 2, c ^ 4 gives these very bits)
ADC_HD float mlp_join8(float s0, float s1, float s2, float s3, float s4, float s5, float s6, float s7)
{
    return ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7));
}

// exp(r) - 1 for |r| <= 0.35, float64: r + r^2 * sum_{k = 2..14} r^(k-2) / k!
ADC_HD double mlp_expm1_poly(double r)
{
    double q = 1.0 / 87178291200.0;
    q = q * r + 1.0 / 6227020800.0;
    q = q * r + 1.0 / 479001600.0;
    q = q * r + 1.0 / 39916800.0;
    q = q * r + 1.0 / 3628800.0;
    q = q * r + 1.0 / 362880.0;
    q = q * r + 1.0 / 40320.0;
    q = q * r + 1.0 / 5040.0;
    q = q * r + 1.0 / 720.0;
    q = q * r + 1.0 / 120.0;
    q = q * r + 1.0 / 24.0;
    q = q * r + 1.0 / 6.0;
    q = q * r + 1.0 / 2.0;
    return r + (r * r) * q;
}

ADC_HD double mlp_bits_to_double(uint64_t u)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __longlong_as_double((long long)u);
#else
    union { uint64_t u; double d; } v; v.u = u; return v.d;
#endif
}

// float64 exp for |x| <= 700
ADC_HD double mlp_exp64(double x)
{
    const double n = __builtin_rint(x * 1.4426950408889634);
    const double r = (x - n * 0.693145751953125) - n * 1.4286068203094173e-06;
    const double p = mlp_expm1_poly(r);
    return (1.0 + p) * mlp_bits_to_double((uint64_t)((long long)n + 1023) << 52);
}

ADC_HD float mlp_tanh(float x)
{
    if (x != x) return x;
    const double a = __builtin_fabs((double)x);
    double t;
    if (a >= 10.0) t = 1.0;
    else if (a + a < 0.34) {
        const double m = mlp_expm1_poly(a + a);
        t = m / (m + 2.0);
    } else {
        const double e = mlp_exp64(a + a);
        t = 1.0 - 2.0 / (e + 1.0);
    }
    return __builtin_copysignf((float)t, x);
}

ADC_HD float mlp_exp(float x)
{
    if (x != x) return x;
    x = x < -87.0f ? -87.0f : x;
    x = x > 88.0f ? 88.0f : x;
    return (float)mlp_exp64((double)x);
}

ADC_HD float mlp_act(float v, int activation)
{
    if (activation == kMlpTanh) return mlp_tanh(v);
    return v > 0.0f ? v : 0.0f;
}

ADC_HD float mlp_normalize(float x, float shift, float scale)
{
    const float d = x - shift;
    return d * scale;
}

ADC_HD float mlp_clamp_log_std(float ls, int clamp, float lo, float hi)
{
    if (clamp) {
        ls = ls < lo ? lo : ls;
        ls = ls > hi ? hi : ls;
    }
    return ls;
}

// the standard normal of action component a from the four words of draw(key, a / 4, ST_MLP, 0, tick)
ADC_HD uint32_t mlp_word(uint64_t key, uint32_t tick, int a)
{
    const U4 w = draw(key, (uint32_t)(a >> 2), ST_MLP, 0u, tick);
    const int h = a & 3;
    return h == 0 ? w.x : h == 1 ? w.y : h == 2 ? w.z : w.w;
}
ADC_HD float mlp_normal(uint64_t key, uint32_t tick, int a) { return normal_from_word(mlp_word(key, tick, a)); }

ADC_HD float mlp_sample(float mean, float ls, float z, int deterministic)
{
    if (deterministic) return mean;
    const float p = mlp_exp(ls) * z;
    return mean + p;
}

// one term of the log-probability's sum8
ADC_HD float mlp_logp_term(float z, float ls)
{
    const float h = (z * z) * 0.5f;
    return (-h) - ls;
}
ADC_HD float mlp_logp_finish(float sum, int A)
{
    const float c = (float)A * 0.918938517570495605f;
    return sum - c;
}

// the env's bid (float32 of whole cents / 100) from an action component
ADC_HD float mlp_bid(float v, float clip_hi)
{
    v = v > 0.01f ? v : 0.01f;
    if (clip_hi > 0.0f) v = v < clip_hi ? v : clip_hi;
    double c = __builtin_rint((double)v * 100.0);
    c = c >= 1.0 ? c : 1.0;
    c = c < 1.0e9 ? c : 1.0e9;
    return (float)(c / 100.0);
}
ADC_HD float mlp_budget(float v, float budget_override)
{
    if (budget_override > 0.0f) return budget_override;
    return v > 0.01f ? v : 0.01f;
}

// the squashed action the env is given: lo + half * (tanh(u) + 1), three roundings after the tanh
ADC_HD float mlp_squash_half(float lo, float hi)
{
    const float d = hi - lo;
    return 0.5f * d;
}
// n in [-1, 1] (units of the box) to the env's units: lo + half * (n + 1)
ADC_HD float mlp_box(float n, float lo, float half)
{
    const float s = n + 1.0f;
    const float p = half * s;
    return lo + p;
}
ADC_HD float mlp_squash(float u, float lo, float half) { return mlp_box(mlp_tanh(u), lo, half); }

// ---- the bounded act (the header comment's law) ----------------------------------------------------------------------------------
constexpr int kMlpGaussian = 0, kMlpRandom = 1;        // the act's exploration mode
ADC_HD float mlp_clamp_unit(float n)
{
    n = n < -1.0f ? -1.0f : n;
    return n > 1.0f ? 1.0f : n;
}
// the uniform of the warm-up from the word a normal would have been made from
ADC_HD float mlp_uniform_unit(uint32_t w)
{
    const float u = unit_half24(w), v = u + u;
    return (v + v) - 1.0f;
}
// w: mlp_word of the component (read in random mode alone); z: its normal (read in gaussian mode alone)
ADC_HD float mlp_bounded_action(float mean, float ls, float z, uint32_t w, int deterministic, int explore)
{
    if (!deterministic && explore == kMlpRandom) return mlp_uniform_unit(w);
    const float t = mlp_tanh(mean);
    if (deterministic) return t;
    const float p = mlp_exp(ls) * z;
    return mlp_clamp_unit(t + p);
}
ADC_HD float mlp_inv_half(float half) { return 1.0f / half; }
// a teacher's action in the env's units to the box's
ADC_HD float mlp_unbox(float e, float lo, float inv_half)
{
    const float d = e - lo, q = d * inv_half;
    return mlp_clamp_unit(q - 1.0f);
}

// element j of the flat observation row from the engine's output arrays of one env (what k_flatten_obs writes)
ADC_HD float mlp_obs_at(int j, int K, const int32_t *clk, const float *cost, const int32_t *imp, const float *rev, const int32_t *conv,
                        double cum_profit, int32_t days)
{
    if (j < K) return (float)clk[j];
    if (j < 2 * K) return cost[j - K];
    if (j == 2 * K) return (float)cum_profit;
    if (j == 2 * K + 1) return (float)days;
    j -= 2 * K + 2;
    if (j < K) return (float)imp[j];
    if (j < 2 * K) return rev[j - K];
    return (float)conv[j - 2 * K];
}

// ---- observation history (the header comment's law) ------------------------------------------------------------------------
constexpr int kMlpMaxFrames = 8;
constexpr int32_t kMlpHistNone = -2;       // `last` of an env that has not acted since its explicit reset
// `from` as an act on episode day d sees it
ADC_HD int32_t mlp_hist_from(int32_t d, int32_t last, int32_t from)
{
    if (d == 0) return 0;
    if (last != d - 1 && last != d) return d;
    return from;
}
ADC_HD bool mlp_hist_valid(int32_t d, int f, int32_t from) { return d - (int32_t)f >= from; }
// the slot of the frame that the act on episode day d wrote
ADC_HD int mlp_hist_slot(int32_t d, int H) { return (int)(d % (int32_t)H); }
// element i >= D0 of the stacked row of one env: hist is the env's [H][D0]
ADC_HD float mlp_hist_at(int i, int D0, int H, const float *hist, int32_t d, int32_t from)
{
    const int f = i / D0, j = i - f * D0;
    if (!mlp_hist_valid(d, f, from)) return 0.0f;
    return hist[(size_t)mlp_hist_slot(d - (int32_t)f, H) * (size_t)D0 + (size_t)j];
}

// splitmix64
ADC_HD uint64_t mlp_mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// the agent's Philox key from its per-env seed
ADC_HD uint64_t mlp_agent_key(uint64_t seed) { return mlp_mix64(seed ^ 0x1F83D9ABFB41BD6Bull); }
// ... and without per-env seeds: from the engine's seed and the env's global id (env_id_base + env)
ADC_HD uint64_t mlp_default_agent_key(uint64_t engine_seed, uint64_t global_env_id)
{
    return mlp_mix64(engine_seed ^ mlp_mix64(global_env_id + 0x5BE0CD19137E2179ull));
}

// weights are stored chain-major in blocks of 32 inputs: W[j][h] of a layer with n_out outputs sits at
// (((j / 32) * n_out + h) * 8 + j % 8) * 4 + (j / 8) % 4, rows padded to a multiple of 32 with zeros that are never read: one
// 16-byte load gives a lane four consecutive steps of its chain, and the eight lanes of one neuron read 128 consecutive bytes
ADC_HD size_t mlp_weight_index(int j, int h, int n_out)
{
    return ((((size_t)(j >> 5) * (size_t)n_out + (size_t)h) * 8u + (size_t)(j & 7)) << 2) + (size_t)((j >> 3) & 3);
}
ADC_HD size_t mlp_weight_count(int n_in, int n_out) { return (size_t)((n_in + 31) >> 5) * (size_t)n_out * 32u; }

// chain c of sum8 for one neuron, on the host's side of the law (the kernel runs the same mlp_mac steps, one chain per lane)
template <class X>
ADC_HD float mlp_neuron(const float *W, const float *b, int n_in, int n_out, int h, const X &x)
{
    float s[kMlpChains];
    for (int c = 0; c < kMlpChains; ++c) {
        float acc = 0.0f;
        for (int j = c; j < n_in; j += kMlpChains) acc = mlp_mac(acc, W[mlp_weight_index(j, h, n_out)], x(j));
        s[c] = acc;
    }
    return mlp_join8(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]) + b[h];
}

}  // namespace adc
