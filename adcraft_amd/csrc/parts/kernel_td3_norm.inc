// kernel_td3_norm.inc - the running observation and reward normalisers of the off-policy (TD3) learners on the device.  The law
// is adc_td3_norm.h: the record and the replay ring hold raw rows, the batch kernels (kernel_td3.inc / kernel_td3_pop.inc)
// normalise them as they gather them, and the kernels here keep the moments.  The code the host twins adc_td3_norm_obs_host /
// adc_td3_norm_rew_host run.
// (part of the single translation unit adc_engine.hip)
// -------------------------------------------------------------------------------------------------
// Shape.  The observation part is k_obs_norm_chunk_sums as it is (a pure HBM stream over the record's raw rows) and
// k_td3_norm_obs_finish, one lane per (normaliser, column): the join in chunk order, norm_finish_raw, the vectors in place.  The
// reward part is k_td3_norm_scan - k_rew_norm_scan with the discount read from the TD3 tables, one lane per env walking its days
// forward - then k_rew_norm_chunk_sums and k_rew_norm_finish as they are.  An update is these five launches (two or three with
// one part alone) whatever the number of normalisers is.  No atomics; all stores are plain vector stores.

// the chunks joined in order and the rest of the law for raw rows, one lane per (member, column); grid (column tiles, members)
__global__ __launch_bounds__(kObsNormBlock) void k_td3_norm_obs_finish(ObsNormView p, adc::NormConfig cfg, const double *__restrict__ part, int chunks,
                                                                        long long S)
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
    adc::norm_finish_raw(cfg, sx, qx, (int64_t)S, count, mean, m2, shift, scale);
    p.count[at] = count; p.mean[at] = mean; p.m2[at] = m2;
    p.shift[at] = shift; p.scale[at] = scale;
}

// k_rew_norm_scan with the TD3 learner's discount: env's days [t0, T) into g[(env / n) * S + (t - t0) * n + env % n],
// S = (T - t0) * n; gamma is `gamma`, or - mem != null - the env's member's law's (envs_per_member envs each)
__global__ __launch_bounds__(kRewNormBlock) void k_td3_norm_scan(int N, int n, int t0, int T, const float *__restrict__ reward,
                                                                 const uint8_t *__restrict__ term, const uint8_t *__restrict__ trunc, float gamma,
                                                                 const Td3Member *__restrict__ mem, int envs_per_member, double *__restrict__ G,
                                                                 double *__restrict__ g)
{
    const int env = blockIdx.x * kRewNormBlock + threadIdx.x;
    if (env >= N) return;
    const float gm = mem ? mem[env / envs_per_member].law.gamma : gamma;
    const int norm = env / n, local = env - norm * n;
    double *mine = g + (size_t)norm * ((size_t)(T - t0) * (size_t)n) + (size_t)local;
    double carry = G[env];
    for (int t = t0; t < T; ++t) {
        const size_t i = (size_t)t * (size_t)N + (size_t)env;
        mine[(size_t)(t - t0) * (size_t)n] = adc::rew_norm_scan_day(carry, gm, reward[i], term[i] | trunc[i]);
    }
    G[env] = carry;
}

// every replaced member's normalisers become its donor's in one launch: src_of_m[m] is the donor, -1 or m itself keeps m (no
// destination is a source: the host has checked).  A part that does not live has a null count.  The carry is the envs' and stays.
// grid (column tiles, members)
__global__ __launch_bounds__(kObsNormBlock) void k_td3_norm_copy(ObsNormView on, RewNormView rn, const int32_t *__restrict__ src_of_m)
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
