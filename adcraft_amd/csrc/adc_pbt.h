// adc_pbt.h - the law of the population-based training scheduler (PBT: Jaderberg et al. 2017 - truncation selection, copy,
// perturb) over a learner population (adc_engine_pg_pop_*, adc_engine_td3_pop_* or adc_engine_sac_pop_*): a round's fitness, its
// smoothing, the ranking, the donor draw and the explored hyperparameters.  Shared by the device kernel k_pbt_fitness (parts/kernel_pbt.inc),
// the host flow of adc_engine_pbt_step (parts/pbt_api.inc: ranking, draw and explore run on the host, from M doubles) and the
// host twins adc_pbt_fitness_host / adc_pbt_plan_host / adc_pbt_explore_host (adc_shims.cpp); tests/pbt_ref.py (SAC:
// tests/pbt_sac_ref.py) restates these comments in numpy, bit for bit.
//
// Every value below is the result of ONE correctly rounded IEEE operation (-ffp-contract=off); "f64" marks float64.
//
//   fitness    f64: an env's return is the sum over the recorded days t ascending, from +0, of f64(record reward[t][env]); a
//              member's fitness is the sum of its envs' returns, envs ascending, from +0, divided by f64(n), n its envs (adc_es.h's
//              fitness words, applied to the record).  The caller may hand a fitness in instead (a held-out evaluation).
//   smoothing  f64: in round 0, or with fitness_ema == 0: s[m] = f[m]; otherwise s[m] = (f64(ema) * s[m]) + ((1.0 - f64(ema)) * f[m])
//              (a difference, two products, a sum).
//   ranking    members sorted ascending by (s, member index); a NaN below every number, several NaNs by index (adc_es.h's
//              centred-rank order).  rank[m] = the member's place, 0 the worst.
//   selection  q = replace_count, 1 <= q <= M / 2: ranks 0 .. q - 1 are replaced, ranks M - q .. M - 1 are the donors.  No
//              replaced member is a donor: copies never chain, and their order cannot matter.  For a replaced member d:
//              w = draw(pbt key, d, ST_PBT = 18, 0, round); its donor is the member of rank M - q + ((uint64(w.x) * q) >> 32).
//   pbt key    mix64(seed ^ 0xBB67AE8584CAA73B), seed = adc_pbt_config.seed, or the engine's seed when that is 0 (mix64:
//              adc_mlp.h).  Nothing else draws from stage 18; no env, agent or td3 stream moves.
//   explore    for every hyperparameter id h in tuned_mask: v = the donor's value; f = bit h of w.y ? factor_hi : factor_lo;
//              v' = v * f (one float32 product), then v' < lo[h] ? lo[h] : v', then v' > hi[h] ? hi[h] : v'.  Ids outside the
//              mask keep the replaced member's own value.  ids - PG: 0 lr, 1 ent_coef, 2 eps_clip, 3 vf_coef; TD3: 0 actor_lr,
//              1 critic_lr, 2 target_noise, 3 tau, 4 sigma; SAC: 0 actor_lr, 1 critic_lr, 2 alpha_lr, 3 tau, 4 alpha,
//              5 target_entropy (usually negative: the one product and the two compares need no special case).  Id 4 is, for
//              TD3 and SAC alike, the one that lives on the device and moves in the log domain.
//   sigma      TD3's exploration sigma is the member's learner log_std[A] on the device and moves in the log domain: every
//              component becomes the donor's component + (bit 4 of w.y ? log_factor_hi : log_factor_lo) (one float32 sum), then
//              clamped to [lo[4], hi[4]], both in log units, as above.  The two log factors are fields of the configuration
//              (float32(log(factor)) is the caller's to fill): the law calls no log.
//   alpha      SAC's temperature is the member's cell {log_alpha, m, v, alpha} on the device (adc_sac.h).  With id 4 tuned a
//              replaced member's cell becomes: la' = the donor's log_alpha + (bit 4 of w.y ? log_factor_hi : log_factor_lo) (one
//              float32 sum), clamped to [lo[4], hi[4]], both in log units, as above; m and v the donor's; alpha = mlp_exp(la'),
//              the function sac_alpha_step forms it with.  For a member with alpha_lr == 0 this is the search over the fixed
//              temperature itself.  With id 4 untuned the cell is the donor's four floats verbatim.
//   then       a replaced member has its donor's s (and, PG, its donor's step count); it keeps its envs, its agents' keys and
//              ticks, (TD3, SAC) its seed and every field of its configuration that is not a tuned id (SAC's init_alpha is not
//              touched: the cell is state); round = round + 1.
#pragma once
#include "adc_mlp.h"
#include <algorithm>
#include <vector>

namespace adc {

constexpr uint32_t ST_PBT = 18;
constexpr int kPbtPg = 0, kPbtTd3 = 1, kPbtSac = 3;
constexpr int kPbtMaxHp = 8;
constexpr int kPbtPgIds = 4, kPbtTd3Ids = 5, kPbtSigma = 4;
constexpr int kPbtSacIds = 6, kPbtAlpha = 4;

ADC_HD uint64_t pbt_key(uint64_t seed) { return mlp_mix64(seed ^ 0xBB67AE8584CAA73Bull); }

// one day of an env's return; one env of a member's fitness
ADC_HD double pbt_chain(double acc, double x) { return acc + x; }
ADC_HD double pbt_fitness_finish(double acc, int n) { return acc / (double)n; }

ADC_HD double pbt_smooth(float ema, double s, double f, bool first)
{
    if (first || ema == 0.0f) return f;
    const double e = (double)ema, a = e * s, o = 1.0 - e, b = o * f;
    return a + b;
}

ADC_HD U4 pbt_draw(uint64_t key, uint32_t member, uint32_t round) { return draw(key, member, ST_PBT, 0u, round); }
// the donor's rank for a replaced member's draw
ADC_HD int pbt_donor_rank(int M, int q, uint32_t wx) { return M - q + (int)(((uint64_t)wx * (uint64_t)q) >> 32); }

ADC_HD float pbt_clamp(float v, float lo, float hi)
{
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}
ADC_HD float pbt_explore(float donor, int up, float factor_lo, float factor_hi, float lo, float hi)
{
    const float v = donor * (up ? factor_hi : factor_lo);
    return pbt_clamp(v, lo, hi);
}
// ... of one log_std component
ADC_HD float pbt_explore_log(float donor, float log_factor, float lo, float hi)
{
    const float v = donor + log_factor;
    return pbt_clamp(v, lo, hi);
}

// a replaced SAC member's temperature cell {log_alpha, m, v, alpha} from its donor's (id 4 tuned)
ADC_HD void pbt_explore_cell(const float donor[4], float log_factor, float lo, float hi, float out[4])
{
    const float la = pbt_explore_log(donor[0], log_factor, lo, hi);
    out[0] = la; out[1] = donor[1]; out[2] = donor[2]; out[3] = mlp_exp(la);
}

// order[r] = the member of rank r (host only: M values)
inline void pbt_rank(const double *s, int M, std::vector<int> &order)
{
    order.resize((size_t)M);
    for (int m = 0; m < M; ++m) order[(size_t)m] = m;
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        const double fa = s[a], fb = s[b];
        const bool na = fa != fa, nb = fb != fb;
        if (na != nb) return na;                       // a NaN ranks below every number
        if (!na && fa != fb) return fa < fb;
        return a < b;
    });
}

// one round's plan from the smoothed fitness: rank[m]; src[m] = the donor of a replaced member, -1 for a member that is kept;
// bits[m] = the replaced member's w.y (0 for the others)
inline void pbt_plan(uint64_t key, uint32_t round, int q, const double *s, int M, int32_t *rank, int32_t *src, uint32_t *bits)
{
    std::vector<int> order;
    pbt_rank(s, M, order);
    for (int r = 0; r < M; ++r) {
        const int m = order[(size_t)r];
        rank[m] = r; src[m] = -1;
        if (bits) bits[m] = 0u;
    }
    for (int r = 0; r < q; ++r) {
        const int d = order[(size_t)r];
        const U4 w = pbt_draw(key, (uint32_t)d, round);
        src[d] = order[(size_t)pbt_donor_rank(M, q, w.x)];
        if (bits) bits[d] = w.y;
    }
}

}  // namespace adc
