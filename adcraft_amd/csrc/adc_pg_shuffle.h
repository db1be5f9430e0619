// adc_pg_shuffle.h - the law of the PPO / A2C learners' shuffled sample-level minibatches and of target-KL early stopping: an epoch's
// order of a member's recorded samples as a counter-addressed permutation (no sort, no state in HBM), the minibatches cut from it,
// and the rule that ends an update which has moved too far (Stable-Baselines3's target_kl).  Shared by the device kernels
// (parts/kernel_pg_shuffle.inc), the host twins adc_pg_shuffle_order_host / adc_pg_shuffle_stop_host (adc_shims.cpp) and
// tests/pg_shuffle_ref.py, which restates these comments in numpy.  An add-on to adc_pg.h (and adc_pg_kl.h): the law of a gradient
// is theirs with the list of record rows replaced - nothing else of it changes.
//
//   shuffle key  mix64(seed ^ 0xA54FF53A5F1D36F1), seed = adc_pg_shuffle_config.seed, or the engine's seed when that is 0 (mix64:
//                adc_mlp.h; as the td3 key is formed).
//   samples      a member has n_s = T * n recorded samples, T the recorded days and n the member's envs (N for a single learner);
//                sample x is day x / n of the member's env x % n: the record row (x / n) * N + member * n + x % n.
//   permutation  sigma_k of [0, n_s) for tick k: a balanced 4-round Feistel network with cycle walking.  b = the smallest even
//                number >= 2 with 2^b >= n_s; h = b / 2; mask = 2^h - 1.  One application to x < 2^b: L = x >> h, R = x & mask;
//                for round r = 0 .. 3: f = (word x of draw(shuffle key, R, ST_PG_SHUFFLE = 19, r, k)) & mask, then
//                (L, R) = (R, L ^ f); x' = (L << h) | R.  sigma_k(i): apply to i, and again to the result while it is >= n_s.
//                One application is a bijection of [0, 2^b) whatever f is, so the walk returns to [0, n_s) and sigma_k is a
//                bijection of it; 2^b < 4 n_s, so the expected walk is under four applications.
//   order        position i of the epoch's order holds sample sigma_k(i).  Minibatch j of the epoch is the positions
//                [j * mb, min((j + 1) * mb, n_s)), mb = minibatch_samples: ceil(n_s / mb) minibatches, the last may be short and is
//                a mean over its own count (as RLlib's and Stable-Baselines3's last slice is).
//   sum order    within a minibatch sample s is position j * mb + s; adc_pg.h's chunked sums (the gradient's, the statistics') run
//                over s = 0 .. count - 1 in that order, S = count.
//   tick         k = the low 32 bits of the member's optimiser step count at the moment the epoch's order is drawn.  The step
//                count is part of adc_engine_pg_state_get / _set (and the _pop_ ones), which therefore carry all a bit-for-bit
//                resume needs; adc_engine_pg_pop_copy and a PBT round copy the step count, the seed stays the destination's.
//                Consequence: an update that stops before its first step redraws the same order next time, over new data.
//   early stop   target_kl > 0: after a minibatch's statistics have reached the host and BEFORE its optimiser step,
//                approx_kl (adc_pg.h's statistic, float64) > 1.5 * f64(target_kl) (one float64 product) ends the member's update:
//                the step is not taken, the step count does not advance.  target_kl == 0 never stops.
//   statistics   of an update: each the mean over the evaluated minibatches of the last epoch the member began, the stopping
//                minibatch included, summed in order from +0 and divided by their number; the KL add-on's end-of-update adaptation
//                uses the same minibatches.  adc_pg_stats.samples is the last evaluated minibatch's count.
#pragma once
#include "adc_law.h"
#include "adc_mlp.h"
#include "adc_pg.h"
#include <cstdint>

namespace adc {

constexpr uint32_t ST_PG_SHUFFLE = 19;

ADC_HD uint64_t pg_shuffle_key(uint64_t seed) { return mlp_mix64(seed ^ 0xA54FF53A5F1D36F1ull); }

// h = b / 2 for n_s >= 1 samples
ADC_HD uint32_t pg_shuffle_half_bits(uint32_t n_s)
{
    uint32_t h = 1;
    while (h < 16u && (1ull << (2u * h)) < (uint64_t)n_s) ++h;
    return h;
}

// one application of the network to x < 2^(2 h)
ADC_HD uint32_t pg_shuffle_feistel(uint64_t key, uint32_t x, uint32_t h, uint32_t tick)
{
    const uint32_t mask = (1u << h) - 1u;
    uint32_t L = x >> h, R = x & mask;
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) {
        const uint32_t f = draw(key, R, ST_PG_SHUFFLE, r, tick).x & mask;
        const uint32_t t = L ^ f;
        L = R;
        R = t;
    }
    return (L << h) | R;
}

// sigma_tick(i), i < n_s
ADC_HD uint32_t pg_shuffle_sample(uint64_t key, uint32_t i, uint32_t n_s, uint32_t h, uint32_t tick)
{
    uint32_t x = i;
    do x = pg_shuffle_feistel(key, x, h, tick);
    while (x >= n_s);
    return x;
}

// the record row of a member's sample x: n the member's envs, N the engine's
ADC_HD uint32_t pg_shuffle_row(uint32_t x, uint32_t n, uint32_t N, uint32_t member) { return (x / n) * N + member * n + x % n; }

ADC_HD bool pg_shuffle_stop(double approx_kl, float target_kl)
{
    if (!(target_kl > 0.0f)) return false;
    const double bound = 1.5 * (double)target_kl;
    return approx_kl > bound;
}

// what the end of a minibatch decides before its optimiser step, from the minibatch's sums (adc_pg.h's kPgSums) over S samples: the
// early stop above (stop_rule: shuffled minibatches are live - env-block minibatches never stop), then the norm clip's scale.  The
// host-driven update takes it on the host between two launches, the queued update (parts/kernel_pg_queued.inc: k_pg_decide) on the
// device: the same code, the same bits.  A stopping minibatch takes no step: its clip is off and its scale 1.
struct PgDecision {
    int stop, clip;
    float scale;
};
ADC_HD PgDecision pg_decide(float max_grad_norm, float target_kl, int stop_rule, const double *sums, int64_t S)
{
    PgDecision d{0, 0, 1.0f};
    if (stop_rule && pg_shuffle_stop(pg_stats_approx_kl(sums, S), target_kl)) {
        d.stop = 1;
        return d;
    }
    d.clip = max_grad_norm > 0.0f;
    if (d.clip) d.scale = pg_clip_scale(max_grad_norm, pg_stats_grad_norm(sums));
    return d;
}

}  // namespace adc
