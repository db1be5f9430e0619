// kernel_obs_norm.inc - the running observation normaliser on the device: one pass over the rollout record's network inputs
// for the batch moments, and a D-long finish that merges them into the running moments and writes shift / scale where the
// policy kernel reads them.  The arithmetic is adc_norm.h's law, the code the host twin adc_obs_norm_host runs.
// (part of the single translation unit adc_engine.hip)
// -------------------------------------------------------------------------------------------------
// Shape.  k_obs_norm_chunk_sums is a pure HBM stream: lanes run along the columns, so a wavefront reads 256 consecutive bytes
// of a row, and a lane walks the 1024 samples of ONE chunk of its column with two float64 accumulators (the sum, the sum of
// squares: one fused multiply-add with an exact product).  The chain's order is the law's and cannot be split, so what hides
// the memory latency is the other wavefronts (columns / 64 x chunks x members of them) and the loads of the next rows, which
// do not depend on the chain: the loop is unrolled by kObsNormUnroll rows.  A wavefront whose columns all lie past D leaves at
// once, so the 256-wide tile costs nothing over a 64-wide one.  The member is the grid's z; a member's samples follow the law's
// order (day, then its own envs), which is k_pg_pop_chunk_sums' index arithmetic with the division carried as two counters.
// k_obs_norm_finish is one lane per (member, column).  No atomics; all stores are plain vector stores.
struct ObsNormView {
    int64_t *count;                         // [Mn][D] (every column carries its normaliser's count: a lane reads and writes its own)
    double *mean, *m2;                      // [Mn][D]
    float *shift, *scale;                   // [Mn][D]: the vectors the policy kernel reads
    int D;
};

constexpr int kObsNormBlock = 256;
constexpr int kObsNormUnroll = 16;

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

// the chunks joined in order and the rest of the law, one lane per (member, column); grid (column tiles, members)
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
    adc::norm_finish(cfg, sx, qx, (int64_t)S, count, mean, m2, shift, scale);
    p.count[at] = count; p.mean[at] = mean; p.m2[at] = m2;
    p.shift[at] = shift; p.scale[at] = scale;
}

// every replaced member's normaliser becomes its donor's in one launch: src_of_m[m] is the donor, -1 or m itself keeps m (no
// destination is a source: the host has checked); grid (column tiles, members)
__global__ __launch_bounds__(kObsNormBlock) void k_obs_norm_copy(ObsNormView p, const int32_t *__restrict__ src_of_m)
{
    const int col = blockIdx.x * kObsNormBlock + threadIdx.x, member = blockIdx.y;
    if (col >= p.D) return;
    const int src = src_of_m[member];
    if (src < 0 || src == member) return;
    const size_t to = (size_t)member * (size_t)p.D + (size_t)col, from = (size_t)src * (size_t)p.D + (size_t)col;
    p.count[to] = p.count[from]; p.mean[to] = p.mean[from]; p.m2[to] = p.m2[from];
    p.shift[to] = p.shift[from]; p.scale[to] = p.scale[from];
}
