// kernel_norm.inc - the running normalisers on the device: the observation normaliser and the reward normaliser of the PPO / A2C
// learners (the laws are adc_norm.h and adc_rew_norm.h) and those of the off-policy (TD3) learners (adc_td3_norm.h: the record and
// the replay ring hold raw rows, the batch kernels of kernel_td3.inc / kernel_td3_pop.inc normalise them as they gather them).
// One set of kernels keeps the moments of all three; it is the code the host twins adc_obs_norm_host / adc_rew_norm_host /
// adc_pg_gae_norm_host / adc_td3_norm_obs_host / adc_td3_norm_rew_host run.
// (part of the single translation unit adc_engine.hip)
// -------------------------------------------------------------------------------------------------
// Shape, observations.  k_obs_norm_chunk_sums is a pure HBM stream: lanes run along the columns, so a wavefront reads 256
// consecutive bytes of a row, and a lane walks the 1024 samples of ONE chunk of its column with two float64 accumulators (the sum,
// the sum of squares: one fused multiply-add with an exact product).  The chain's order is the law's and cannot be split, so what
// hides the memory latency is the other wavefronts (columns / 64 x chunks x members of them) and the loads of the next rows, which
// do not depend on the chain: the loop is unrolled by kObsNormUnroll rows.  A wavefront whose columns all lie past D leaves at
// once, so the 256-wide tile costs nothing over a 64-wide one.  The member is the grid's z; a member's samples follow the law's
// order (day, then its own envs), which is k_pg_pop_chunk_sums' index arithmetic with the division carried as two counters.
// k_obs_norm_finish is one lane per (member, column): the join in chunk order, norm_finish - RAW for the TD3 learners' raw rows,
// through the vectors in force otherwise - and the vectors in place.
// Shape, rewards.  k_rew_norm_scan is one lane per env walking its days forward: lanes run along the envs, so a wavefront reads 64
// consecutive rewards of a day and writes 64 consecutive returns of the float64 scratch, which is laid out in the law's sample
// order ([normaliser][day - t0][local env]); the env's carry G lives in HBM between updates.  The discount is the learner's own:
// a PPO / A2C member's or a TD3 member's (norm_member_gamma).  k_rew_norm_chunk_sums is k_pg_pop_chunk_sums' sibling for float64
// input: grid (chunks / block, normalisers), one lane per chunk of 1024 samples with two float64 accumulators (the sum, the sum of
// rounded squares), 32 loads in flight ahead of the chain; partials [normaliser][chunk][2].  k_rew_norm_finish is one lane per
// normaliser: the join in chunk order, the merge, the multiplier in place.
// An update is two launches for the observations and three for the rewards whatever the number of normalisers is.  No atomics; all
// stores are plain vector stores.
struct ObsNormView {
    int64_t *count;                         // [Mn][D] (every column carries its normaliser's count: a lane reads and writes its own)
    double *mean, *m2;                      // [Mn][D]
    float *shift, *scale;                   // [Mn][D]: the vectors the policy kernel reads
    int D;
};
struct RewNormView {
    int64_t *count;                         // [Mn]
    double *mean, *m2;                      // [Mn]
    float *scale;                           // [Mn]: the multiplier the GAE kernels and the TD3 target read
    double *G;                              // [N]: every env's running discounted return
};

constexpr int kObsNormBlock = 256;
constexpr int kObsNormUnroll = 16;
constexpr int kRewNormBlock = 256;
constexpr int kRewNormUnroll = 32;

// partials part[((member * chunks + chunk) * 2 + {0: sum, 1: squares}) * D + col] of the days [t0, t0 + days) of obs [T][N][D];
// grid (column tiles, chunks, members); member m's sample i is day t0 + i / n, env m * n + i % n
__global__ __launch_bounds__(kObsNormBlock) void k_obs_norm_chunk_sums(const float *__restrict__ obs, int D, int N, int n, int t0, long long S,
                                                                       double *__restrict__ part)
{
    const int col = blockIdx.x * kObsNormBlock + threadIdx.x;
    if (col >= D) return;
    const long long chunk = blockIdx.y, chunks = gridDim.y;
    const int member = blockIdx.z;
    const long long i0 = chunk * adc::kPgChunk;
    const int cnt = (int)(i0 + adc::kPgChunk < S ? adc::kPgChunk : S - i0);
    int t = t0 + (int)(i0 / n), local = (int)(i0 % n);
    const size_t env0 = (size_t)member * (size_t)n;
    double acc_s = 0.0, acc_q = 0.0;
    int i = 0;
    for (; i + kObsNormUnroll <= cnt; i += kObsNormUnroll) {
        float x[kObsNormUnroll];
#pragma unroll
        for (int u = 0; u < kObsNormUnroll; ++u) {
            x[u] = obs[((size_t)t * (size_t)N + env0 + (size_t)local) * (size_t)D + (size_t)col];
            if (++local == n) { local = 0; ++t; }
        }
#pragma unroll
        for (int u = 0; u < kObsNormUnroll; ++u) {
            acc_s = adc::norm_chain_sum(acc_s, x[u]);
            acc_q = adc::pg_chain_mac(acc_q, x[u], x[u]);
        }
    }
    for (; i < cnt; ++i) {
        const float x = obs[((size_t)t * (size_t)N + env0 + (size_t)local) * (size_t)D + (size_t)col];
        if (++local == n) { local = 0; ++t; }
        acc_s = adc::norm_chain_sum(acc_s, x);
        acc_q = adc::pg_chain_mac(acc_q, x, x);
    }
    double *mine = part + (((size_t)member * (size_t)chunks + (size_t)chunk) * 2u) * (size_t)D + (size_t)col;
    mine[0] = acc_s;
    mine[D] = acc_q;
}

// the chunks joined in order and the rest of the law, one lane per (member, column); grid (column tiles, members).  RAW: the rows
// are raw observations (adc_td3_norm.h), there is no back-conversion through the vectors in force
template <bool RAW>
__global__ __launch_bounds__(kObsNormBlock) void k_obs_norm_finish(ObsNormView p, adc::NormConfig cfg, const double *__restrict__ part, int chunks, long long S)
{
    const int col = blockIdx.x * kObsNormBlock + threadIdx.x, member = blockIdx.y;
    if (col >= p.D) return;
    const size_t D = (size_t)p.D;
    const double *mine = part + (size_t)member * (size_t)chunks * 2u * D + (size_t)col;
    double sx = 0.0, qx = 0.0;
    for (int c = 0; c < chunks; ++c) {
        sx = sx + mine[(size_t)c * 2u * D];
        qx = qx + mine[(size_t)c * 2u * D + D];
    }
    const size_t at = (size_t)member * D + (size_t)col;
    int64_t count = p.count[at];
    double mean = p.mean[at], m2 = p.m2[at];
    float shift = p.shift[at], scale = p.scale[at];
    adc::norm_finish(cfg, RAW, sx, qx, (int64_t)S, count, mean, m2, shift, scale);
    p.count[at] = count; p.mean[at] = mean; p.m2[at] = m2;
    p.shift[at] = shift; p.scale[at] = scale;
}

// the discount of a learner's member: a PPO / A2C member's, a TD3 member's law's
__device__ inline float norm_member_gamma(const PgMember &m) { return m.gamma; }
__device__ inline float norm_member_gamma(const Td3Member &m) { return m.law.gamma; }

// env's days [t0, T) into g[(env / n) * S + (t - t0) * n + env % n], S = (T - t0) * n; gamma is `gamma`, or - mem != null - the
// env's member's (envs_per_member envs each)
template <typename Member>
__global__ __launch_bounds__(kRewNormBlock) void k_rew_norm_scan(int N, int n, int t0, int T, const float *__restrict__ reward,
                                                                 const uint8_t *__restrict__ term, const uint8_t *__restrict__ trunc, float gamma,
                                                                 const Member *__restrict__ mem, int envs_per_member, double *__restrict__ G,
                                                                 double *__restrict__ g)
{
    const int env = blockIdx.x * kRewNormBlock + threadIdx.x;
    if (env >= N) return;
    const float gm = mem ? norm_member_gamma(mem[env / envs_per_member]) : gamma;
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

// every replaced member's normalisers become its donor's in one launch: src_of_m[m] is the donor, -1 or m itself keeps m (no
// destination is a source: the host has checked).  A part that does not live has a null count.  The carry is the envs' and stays.
// grid (column tiles, members)
__global__ __launch_bounds__(kObsNormBlock) void k_norm_copy(ObsNormView on, RewNormView rn, const int32_t *__restrict__ src_of_m)
{
    const int col = blockIdx.x * kObsNormBlock + threadIdx.x, member = blockIdx.y;
    const int src = src_of_m[member];
    if (src < 0 || src == member) return;
    if (on.count && col < on.D) {
        const size_t to = (size_t)member * (size_t)on.D + (size_t)col, from = (size_t)src * (size_t)on.D + (size_t)col;
        on.count[to] = on.count[from]; on.mean[to] = on.mean[from]; on.m2[to] = on.m2[from];
        on.shift[to] = on.shift[from]; on.scale[to] = on.scale[from];
    }
    if (rn.count && col == 0) {
        rn.count[member] = rn.count[src]; rn.mean[member] = rn.mean[src]; rn.m2[member] = rn.m2[src]; rn.scale[member] = rn.scale[src];
    }
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
