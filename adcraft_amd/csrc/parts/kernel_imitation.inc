// kernel_imitation.inc - imitation learning on the device (adc_imitation.h): the teacher's action into the record's slot of a
// teacher day, and the sample pass of the imitation loss.
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

__global__ __launch_bounds__(kPgBlock) void k_im_sample(PgView p, adc::ImLaw im)
{
    pg_sample_body<false, false, true>(p, p.net, p.log_std, p.loss, p.n0, blockIdx.x, blockIdx.x, PgKlView{}, adc::PgKl{}, 0, nullptr, im);
}
