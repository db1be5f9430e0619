// kernel_imitation.inc - imitation learning on the device (adc_imitation.h): the teacher's action into the record's slot of a
// teacher day, the label, played action and mask of a DAgger day (adc_dagger.h), and the sample pass of the imitation loss.
// (part of the single translation unit adc_engine.hip)
// -------------------------------------------------------------------------------------------------
// k_im_sample is k_pg_sample with the imitation loss in the surrogate's place: pg_sample_body's instantiation kIm, the same
// workgroup per sample, the same LDS carve (the one without the KL add-on's rows), the same scratch rows acts / deltas / pieces in
// the layout k_pg_wgrad reads.  Everything after it - k_pg_wgrad, k_pg_grad_join, the sums, the norm clip, k_pg_update - is the
// policy-gradient trainer's as it is.

// The record's slot of a teacher day: action[env][0] = the budget and action[env][1 + k] = the bid of keyword k the step is about
// to consume (the float32 values in the engine's action buffers), logp = +0.  One lane per (env, component); `bids` / `budgets` /
// `action` / `logp` start at the view's first env.
__global__ void k_teach_record(int n, int K, const float *__restrict__ bids, const float *__restrict__ budgets, float *__restrict__ action,
                               float *__restrict__ logp)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int A = K + 1;
    if (i >= (long long)n * A) return;
    const int env = (int)(i / A), a = (int)(i % A);
    if (a == 0) {
        action[i] = budgets[env];
        logp[env] = 0.0f;
    } else action[i] = bids[(size_t)env * (size_t)K + (size_t)(a - 1)];
}

// ... under the bounded act (adc_mlp.h "bounded"): the slot holds the teacher's action in units of the box, n = mlp_unbox(e), so that
// a bounded TD3 learner's critics read a teacher day as they read the learner's own.  lo / inv_half: [A]
__global__ void k_teach_record_bounded(int n, int K, const float *__restrict__ bids, const float *__restrict__ budgets,
                                       const float *__restrict__ lo, const float *__restrict__ inv_half, float *__restrict__ action,
                                       float *__restrict__ logp)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int A = K + 1;
    if (i >= (long long)n * A) return;
    const int env = (int)(i / A), a = (int)(i % A);
    const float ea = a == 0 ? budgets[env] : bids[(size_t)env * (size_t)K + (size_t)(a - 1)];
    action[i] = adc::mlp_unbox(ea, lo[a], inv_half[a]);
    if (a == 0) logp[env] = 0.0f;
}

// The record's slot of a DAgger day, the played action and the mask (adc_dagger.h).  One lane per (env, component), as above: the
// label is what k_teach_record / k_teach_record_bounded would write; where the env's coin picks the teacher the teacher's
// env-ready component goes over the learner's in the scratch the step is about to consume (`sbids` / `sbudget`), elsewhere the
// scratch keeps the learner's; mask[env] = the coin.  Every lane of an env draws the coin again (one Philox call): nothing is
// shared between lanes.  `tick` is behind the day's act: the coin's tick is tick[env] - 1.  All pointers start at the view's first env.
struct DaggerMix {
    const uint64_t *key;                    // [n] the agents' keys
    const uint32_t *tick;                   // [n] ... and ticks, moved on by the act
    uint64_t threshold;                     // bernoulli_threshold(beta)
    const float *bids, *budgets;            // [n][K], [n] the teacher's action (the engine's action buffers)
    float *sbids, *sbudget;                 // [n][K], [n] the learner's env-ready action (the scratch)
    float *action, *logp;                   // [n][K + 1], [n] the record's slot
    uint8_t *mask;                          // [n] the mask's row
};
template <bool kBounded>
__device__ __forceinline__ void dagger_mix_body(int n, int K, const DaggerMix &d, const float *__restrict__ lo, const float *__restrict__ inv_half)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int A = K + 1;
    if (i >= (long long)n * A) return;
    const int env = (int)(i / A), a = (int)(i % A);
    const size_t kw = (size_t)env * (size_t)K + (size_t)(a > 0 ? a - 1 : 0);
    const bool teacher = adc::dagger_coin(d.key[env], d.tick[env] - 1u, d.threshold);
    const float ea = a == 0 ? d.budgets[env] : d.bids[kw];
    if constexpr (kBounded) d.action[i] = adc::mlp_unbox(ea, lo[a], inv_half[a]);
    else d.action[i] = ea;
    if (a == 0) {
        d.logp[env] = 0.0f;
        d.mask[env] = teacher ? 1 : 0;
        if (teacher) d.sbudget[env] = ea;
    } else if (teacher) d.sbids[kw] = ea;
}
__global__ void k_dagger_mix(int n, int K, DaggerMix d) { dagger_mix_body<false>(n, K, d, nullptr, nullptr); }
__global__ void k_dagger_mix_bounded(int n, int K, DaggerMix d, const float *__restrict__ lo, const float *__restrict__ inv_half)
{
    dagger_mix_body<true>(n, K, d, lo, inv_half);
}

__global__ __launch_bounds__(kPgBlock) void k_im_sample(PgView p, adc::ImLaw im)
{
    pg_sample_body<false, false, true>(p, p.net, p.log_std, p.loss, p.n0, blockIdx.x, blockIdx.x, PgKlView{}, adc::PgKl{}, 0, nullptr, im);
}
