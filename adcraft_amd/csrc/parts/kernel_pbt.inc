// kernel_pbt.inc - population-based training over a learner population (adc_engine_pbt_*; the law is adc_pbt.h): the members'
// fitness from the rollout record where it lies, and the exploit - every replaced member made a copy of its donor from a
// (dst, src) table in a fixed number of launches, whatever the number of pairs.  No destination is a source (the plan's
// selection, checked by the host for a plan handed in), so a launch reads donors and writes destinations and the pairs' order
// cannot matter; a donor read by several destinations is only read.  No atomics; all stores are plain vector stores.  Over a SAC
// population (kind ADC_PBT_SAC) k_pbt_exploit and k_pbt_exploit_ring run as they are and k_pbt_exploit_cell copies or explores the
// temperature cells.
// (part of the single translation unit adc_engine.hip)
struct PbtPair {
    int dst, src;
    int sigma;                              // TD3: dst's log_std = clamp(src's log_std + log_factor); else dst keeps its own
    float log_factor;
};

constexpr int kPbtBlock = 256;

// member blockIdx.x: its envs' returns one lane per env, each chaining over the T recorded days in day order; then the member's
// chain over its envs in env order (one lane).  reward is the record's [T][N]; ret [N] and fit [M] are float64
__global__ __launch_bounds__(kPbtBlock) void k_pbt_fitness(int N, int T, int envs_per_member, const float *__restrict__ reward, double *ret, double *fit)
{
    const int member = blockIdx.x, n = envs_per_member;
    const size_t env0 = (size_t)member * (size_t)n;
    for (int i = threadIdx.x; i < n; i += kPbtBlock) {
        double acc = 0.0;
        for (int t = 0; t < T; ++t) acc = adc::pbt_chain(acc, (double)reward[(size_t)t * (size_t)N + env0 + (size_t)i]);
        ret[env0 + (size_t)i] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc = adc::pbt_chain(acc, ret[env0 + (size_t)i]);
        fit[member] = adc::pbt_fitness_finish(acc, n);
    }
}

// pair blockIdx.y: parameter p of the [M][Q] vector `flat` (and of its moments, when it has them) from src's row into dst's, and
// dst's chain-major store rebuilt from it (L is member 0's stores, a member's `stride` floats further: what k_pg_pop_params_copy
// does for one member).  With log_std0 (TD3's actor vector alone; member 0's log_std, a member's ls_stride floats further) the
// pair's block 0 also writes dst's explored log_std from src's
__global__ __launch_bounds__(kPgBlock) void k_pbt_exploit(PgLayout L, size_t stride, float *flat, float *mom_m, float *mom_v, const PbtPair *__restrict__ pairs,
                                                          float *log_std0, size_t ls_stride, int A, float ls_lo, float ls_hi)
{
    const PbtPair pr = pairs[blockIdx.y];
    const size_t src = (size_t)pr.src, dst = (size_t)pr.dst;
    if (log_std0 && pr.sigma && blockIdx.x == 0)
        for (int a = threadIdx.x; a < A; a += kPgBlock)
            log_std0[dst * ls_stride + (size_t)a] = adc::pbt_explore_log(log_std0[src * ls_stride + (size_t)a], pr.log_factor, ls_lo, ls_hi);
    const int p = blockIdx.x * kPgBlock + threadIdx.x;
    if (p >= L.Q) return;
    const size_t from = src * (size_t)L.Q + (size_t)p, to = dst * (size_t)L.Q + (size_t)p;
    const float t = flat[from];
    flat[to] = t;
    if (mom_m) {
        mom_m[to] = mom_m[from];
        mom_v[to] = mom_v[from];
    }
    *(pg_param_slot(L, p) + dst * stride) = t;
}

// `bytes` bytes from s to d by the grid's lanes (lane of lanes): 16-byte stores on d's 16-byte boundaries, single bytes before the
// first and after the last; a 16-byte store's loads are one 16-byte load, four 4-byte loads or sixteen bytes, as s's own alignment
// at that point allows.  Nothing here is assumed to be a multiple of 16: not the pointers, not their distance, not the length
__device__ __forceinline__ void pbt_copy_bytes(uint8_t *d, const uint8_t *s, size_t bytes, size_t lane, size_t lanes)
{
    size_t head = (size_t)((16u - (unsigned)((uintptr_t)d & 15u)) & 15u);
    if (head > bytes) head = bytes;
    for (size_t i = lane; i < head; i += lanes) d[i] = s[i];
    const size_t body = (bytes - head) / 16u;
    uint8_t *db = d + head;
    const uint8_t *sb = s + head;
    const unsigned mis = (unsigned)((uintptr_t)sb & 15u);
    if (mis == 0u) {
        for (size_t i = lane; i < body; i += lanes) *reinterpret_cast<uint4 *>(db + 16u * i) = *reinterpret_cast<const uint4 *>(sb + 16u * i);
    } else if ((mis & 3u) == 0u) {
        for (size_t i = lane; i < body; i += lanes) {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(sb + 16u * i);
            uint4 v;
            v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
            *reinterpret_cast<uint4 *>(db + 16u * i) = v;
        }
    } else {
        for (size_t i = lane; i < body; i += lanes) {
            const uint8_t *b = sb + 16u * i;
            uint32_t w[4];
            for (int k = 0; k < 4; ++k)
                w[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
            uint4 v;
            v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
            *reinterpret_cast<uint4 *>(db + 16u * i) = v;
        }
    }
    for (size_t i = head + 16u * body + lane; i < bytes; i += lanes) d[i] = s[i];
}

// pair blockIdx.y, ring array blockIdx.z (x, a, r, x2, done; 5: gn, launched under n-step returns alone) of C slots: src's into dst's.  Rows are D = 5K + 2 and A = K + 1
// floats and done is bytes, a member's arrays start C rows after the previous member's: no alignment beyond the element's holds
__global__ __launch_bounds__(kPbtBlock) void k_pbt_exploit_ring(const Td3Member *__restrict__ mem, const PbtPair *__restrict__ pairs, size_t C, int D, int A)
{
    const PbtPair pr = pairs[blockIdx.y];
    const Td3Ring s = mem[pr.src].ring, d = mem[pr.dst].ring;
    const size_t lane = (size_t)blockIdx.x * kPbtBlock + threadIdx.x, lanes = (size_t)gridDim.x * kPbtBlock;
    uint8_t *dp;
    const uint8_t *sp;
    size_t bytes;
    switch (blockIdx.z) {
    case 0: dp = reinterpret_cast<uint8_t *>(d.x); sp = reinterpret_cast<const uint8_t *>(s.x); bytes = C * (size_t)D * 4u; break;
    case 1: dp = reinterpret_cast<uint8_t *>(d.a); sp = reinterpret_cast<const uint8_t *>(s.a); bytes = C * (size_t)A * 4u; break;
    case 2: dp = reinterpret_cast<uint8_t *>(d.r); sp = reinterpret_cast<const uint8_t *>(s.r); bytes = C * 4u; break;
    case 3: dp = reinterpret_cast<uint8_t *>(d.x2); sp = reinterpret_cast<const uint8_t *>(s.x2); bytes = C * (size_t)D * 4u; break;
    case 5: dp = reinterpret_cast<uint8_t *>(d.gn); sp = reinterpret_cast<const uint8_t *>(s.gn); bytes = C * 4u; break;
    default: dp = d.done; sp = s.done; bytes = C; break;
    }
    pbt_copy_bytes(dp, sp, bytes, lane, lanes);
}

// SAC: one lane per pair, the temperature cells [M][4] = {log_alpha, m, v, alpha}: dst's cell is src's four floats verbatim, or -
// the pair's `sigma` flag set (id 4 tuned) - the law's explored cell: log_alpha shifted by log_factor and clamped to [la_lo, la_hi],
// src's m and v, alpha = mlp_exp of the new log_alpha.  One 16-byte load of the donor's cell, one 16-byte store (a cell is four
// floats at a 16-byte boundary: the array is an allocation of its own)
__global__ __launch_bounds__(kPbtBlock) void k_pbt_exploit_cell(int npairs, float *cells, const PbtPair *__restrict__ pairs, float la_lo, float la_hi)
{
    const int j = blockIdx.x * kPbtBlock + threadIdx.x;
    if (j >= npairs) return;
    const PbtPair pr = pairs[j];
    const float4 s = *reinterpret_cast<const float4 *>(cells + (size_t)pr.src * 4u);
    const float donor[4] = {s.x, s.y, s.z, s.w};
    float out[4] = {s.x, s.y, s.z, s.w};
    if (pr.sigma) adc::pbt_explore_cell(donor, pr.log_factor, la_lo, la_hi, out);
    *reinterpret_cast<float4 *>(cells + (size_t)pr.dst * 4u) = make_float4(out[0], out[1], out[2], out[3]);
}
