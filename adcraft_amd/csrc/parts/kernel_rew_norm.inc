// kernel_rew_norm.inc - the running reward normaliser on the device: a forward scan of the rollout record's rewards into the
// discounted returns, their chunked moments, and a finish that merges them into the running moments and writes the reward
// multiplier where the GAE kernels below read it.  The arithmetic is adc_rew_norm.h's law, the code the host twins
// adc_rew_norm_host / adc_pg_gae_norm_host run.
// (part of the single translation unit adc_engine.hip)
// -------------------------------------------------------------------------------------------------
// Shape.  k_rew_norm_scan is one lane per env walking its days forward: lanes run along the envs, so a wavefront reads 64
// consecutive rewards of a day and writes 64 consecutive returns of the float64 scratch, which is laid out in the law's sample
// order ([normaliser][day - t0][local env]); the env's carry G lives in HBM between updates.  k_rew_norm_chunk_sums is
// k_pg_pop_chunk_sums' sibling for float64 input: grid (chunks / block, normalisers), one lane per chunk of 1024 samples with
// two float64 accumulators (the sum, the sum of rounded squares), 32 loads in flight ahead of the chain; partials [normaliser][chunk][2].
// k_rew_norm_finish is one lane per normaliser: the join in chunk order, the merge, the multiplier in place.  An update is these
// three launches whatever the number of normalisers is.  No atomics; all stores are plain vector stores.
struct RewNormView {
    int64_t *count;                         // [Mn]
    double *mean, *m2;                      // [Mn]
    float *scale;                           // [Mn]: the multiplier the GAE kernels read
    double *G;                              // [N]: every env's running discounted return
};

constexpr int kRewNormBlock = 256;
constexpr int kRewNormUnroll = 32;

// env's days [t0, T) into g[(env / n) * S + (t - t0) * n + env % n], S = (T - t0) * n; gamma is `gamma`, or - mem != null - the
// env's member's (envs_per_member envs each)
__global__ __launch_bounds__(kRewNormBlock) void k_rew_norm_scan(int N, int n, int t0, int T, const float *__restrict__ reward,
                                                                 const uint8_t *__restrict__ term, const uint8_t *__restrict__ trunc, float gamma,
                                                                 const PgMember *__restrict__ mem, int envs_per_member, double *__restrict__ G,
                                                                 double *__restrict__ g)
{
    const int env = blockIdx.x * kRewNormBlock + threadIdx.x;
    if (env >= N) return;
    const float gm = mem ? mem[env / envs_per_member].gamma : gamma;
    const int norm = env / n, local = env - norm * n;
    double *mine = g + (size_t)norm * ((size_t)(T - t0) * (size_t)n) + (size_t)local;
    double carry = G[env];
    for (int t = t0; t < T; ++t) {
        const size_t i = (size_t)t * (size_t)N + (size_t)env;
        mine[(size_t)(t - t0) * (size_t)n] = adc::rew_norm_scan_day(carry, gm, reward[i], term[i] | trunc[i]);
    }
    G[env] = carry;
}

// partials part[(normaliser * chunks + chunk) * 2 + {0: sum, 1: squares}] of g [normalisers][S]; grid (chunk blocks, normalisers)
__global__ __launch_bounds__(kRewNormBlock) void k_rew_norm_chunk_sums(const double *__restrict__ g, long long S, int chunks, double *__restrict__ part)
{
    const int chunk = blockIdx.x * kRewNormBlock + threadIdx.x, norm = blockIdx.y;
    if (chunk >= chunks) return;
    const long long i0 = (long long)chunk * adc::kPgChunk;
    const int cnt = (int)(i0 + adc::kPgChunk < S ? adc::kPgChunk : S - i0);
    const double *src = g + (size_t)norm * (size_t)S + (size_t)i0;
    double acc_s = 0.0, acc_q = 0.0;
    int i = 0;
    for (; i + kRewNormUnroll <= cnt; i += kRewNormUnroll) {
        double x[kRewNormUnroll];
#pragma unroll
        for (int u = 0; u < kRewNormUnroll; ++u) x[u] = src[i + u];
#pragma unroll
        for (int u = 0; u < kRewNormUnroll; ++u) {
            acc_s = adc::rew_norm_chain_sum(acc_s, x[u]);
            acc_q = adc::rew_norm_chain_sq(acc_q, x[u]);
        }
    }
    for (; i < cnt; ++i) {
        const double x = src[i];
        acc_s = adc::rew_norm_chain_sum(acc_s, x);
        acc_q = adc::rew_norm_chain_sq(acc_q, x);
    }
    double *mine = part + ((size_t)norm * (size_t)chunks + (size_t)chunk) * 2u;
    mine[0] = acc_s;
    mine[1] = acc_q;
}

// the chunks joined in order and the rest of the law, one lane per normaliser
__global__ __launch_bounds__(kRewNormBlock) void k_rew_norm_finish(RewNormView p, int Mn, adc::NormConfig cfg, const double *__restrict__ part, int chunks,
                                                                   long long S)
{
    const int norm = blockIdx.x * kRewNormBlock + threadIdx.x;
    if (norm >= Mn) return;
    const double *mine = part + (size_t)norm * (size_t)chunks * 2u;
    double sx = 0.0, qx = 0.0;
    for (int c = 0; c < chunks; ++c) {
        sx = sx + mine[(size_t)c * 2u];
        qx = qx + mine[(size_t)c * 2u + 1u];
    }
    int64_t count = p.count[norm];
    double mean = p.mean[norm], m2 = p.m2[norm];
    float scale = p.scale[norm];
    adc::rew_norm_finish(cfg, sx, qx, (int64_t)S, count, mean, m2, scale);
    p.count[norm] = count; p.mean[norm] = mean; p.m2[norm] = m2; p.scale[norm] = scale;
}

// every replaced member's normaliser becomes its donor's in one launch: src_of_m[m] is the donor, -1 or m itself keeps m (no
// destination is a source: the host has checked).  The carry is the envs' and stays.
__global__ __launch_bounds__(kRewNormBlock) void k_rew_norm_copy(RewNormView p, int Mn, const int32_t *__restrict__ src_of_m)
{
    const int member = blockIdx.x * kRewNormBlock + threadIdx.x;
    if (member >= Mn) return;
    const int src = src_of_m[member];
    if (src < 0 || src == member) return;
    p.count[member] = p.count[src]; p.mean[member] = p.mean[src]; p.m2[member] = p.m2[src]; p.scale[member] = p.scale[src];
}

// a host-initiated reset of the envs (all of them, or the masked ones) ends their running return
__global__ __launch_bounds__(kRewNormBlock) void k_rew_norm_carry_reset(int N, const uint8_t *__restrict__ mask, double *__restrict__ G)
{
    const int env = blockIdx.x * kRewNormBlock + threadIdx.x;
    if (env >= N || (mask && !mask[env])) return;
    G[env] = 0.0;
}

// k_pg_gae under a normaliser: the reward times scale[0], clipped (adc_rew_norm.h); one lane per env, walking the record backwards
__global__ void k_rew_norm_gae(int N, int T, const float *__restrict__ reward, const uint8_t *__restrict__ term, const uint8_t *__restrict__ trunc,
                               const float *__restrict__ value, const float *__restrict__ boot, float gamma, float gl, float reward_scale,
                               const float *__restrict__ scale, float clip, float *__restrict__ adv_out, float *__restrict__ ret_out)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N) return;
    const float sc = scale[0];
    float adv = 0.0f, next = boot[env];
    for (int t = T - 1; t >= 0; --t) {
        const size_t i = (size_t)t * (size_t)N + (size_t)env;
        const float v = value[i];
        const float a = adc::rew_norm_gae_day(reward[i], reward_scale, sc, clip, term[i] | trunc[i], v, next, gamma, gl, adv);
        adv_out[i] = a;
        ret_out[i] = a + v;
        next = v;
    }
}

// k_pg_pop_gae under a normaliser: the env's member's constants, the multiplier of the env's normaliser (envs_per_norm envs
// each: N for the shared one)
__global__ void k_rew_norm_pop_gae(int N, int T, int envs_per_member, const PgMember *__restrict__ mem, const float *__restrict__ reward,
                                   const uint8_t *__restrict__ term, const uint8_t *__restrict__ trunc, const float *__restrict__ value,
                                   const float *__restrict__ boot, const float *__restrict__ scale, int envs_per_norm, float clip,
                                   float *__restrict__ adv_out, float *__restrict__ ret_out)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N) return;
    const PgMember &c = mem[env / envs_per_member];
    const float gamma = c.gamma, gl = c.gl, reward_scale = c.reward_scale, sc = scale[env / envs_per_norm];
    float adv = 0.0f, next = boot[env];
    for (int t = T - 1; t >= 0; --t) {
        const size_t i = (size_t)t * (size_t)N + (size_t)env;
        const float v = value[i];
        const float a = adc::rew_norm_gae_day(reward[i], reward_scale, sc, clip, term[i] | trunc[i], v, next, gamma, gl, adv);
        adv_out[i] = a;
        ret_out[i] = a + v;
        next = v;
    }
}
