// kernel_per.inc - prioritised replay on the device: a radix-64 sum tree over the replay ring's slots, sampled by one wave per
// batch element, the batch's importance weights, the leaves' update from the critics' errors and the touched nodes' rebuild.
// The arithmetic is adc_per.h's law, the code the host twins adc_per_*_host run.  The batch kernels of kernel_td3.inc /
// kernel_sac.inc and of their population twins read the slots and weights written here in place of td3_batch_index.
// (part of the single translation unit adc_engine.hip)
// -------------------------------------------------------------------------------------------------
// Shape.  A node's 64 children are one coalesced load, a lane each; their inclusive scan is six rounds of a lane shuffle and an
// add in float64 (Hillis-Steele, the law's order), the child a ballot.  Every level is padded with zeros to a multiple of 64, so
// the load needs no bound.  A node is only ever written as the last lane of that scan over its children: two waves that
// rebuild the same node write identical values.  The member of a population is blockIdx.y: its tree, top and batch buffers lie
// `*_stride` further per member, its key is its row's of the Td3Member table; a solo learner is member 0 of one.  No atomics;
// all stores are plain vector stores.
struct PerView {
    float *leaf;                            // [M][roundup(C, 64)]
    float *top;                             // [M]
    double *node[adc::kPerMaxLevels + 1];   // [1 .. levels]: [M][roundup(n_l, 64)]
    long long n[adc::kPerMaxLevels + 1];    // [0 .. levels]: the levels' counts, n[0] = C
    size_t stride[adc::kPerMaxLevels + 1];  // [0 .. levels]: elements between two members' arrays of a level
    int levels, B;
    int32_t *slot;                          // [M][B] the update's slots
    float *leaf_b, *w, *absd, *pab;         // [M][B] the sampled leaves, the weights; [M][B][2] |d_1|, |d_2|; [M][B] pa(p_b)
};

// member m's view (the host shifts a view so for a launch over one member)
__host__ __device__ inline PerView per_member(PerView t, size_t m)
{
    t.leaf += m * t.stride[0];
    t.top += m;
    for (int l = 1; l <= adc::kPerMaxLevels; ++l) t.node[l] += m * t.stride[l];
    const size_t at = m * (size_t)t.B;
    t.slot += at; t.leaf_b += at; t.w += at; t.absd += 2 * at; t.pab += at;
    return t;
}

// lane i's inclusive prefix of the wave's values, the law's order
__device__ __forceinline__ double per_scan(double v, int lane)
{
    double c = v;
#pragma unroll
    for (int s = 1; s < adc::kPerRadix; s += s) {
        const double t = __shfl_up(c, (unsigned)s, 64);
        if (lane >= s) c = c + t;
    }
    return c;
}

// slot and leaf of batch element blockIdx.x for update `update`: one wave walks from the root to a leaf
__global__ __launch_bounds__(64) void k_per_sample(PerView tv, uint64_t key, const Td3Member *__restrict__ mem, uint32_t update, uint32_t size)
{
    const PerView t = per_member(tv, blockIdx.y);
    const int lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const double u53 = adc::per_u53(mem ? mem[blockIdx.y].key : key, b, update);
    double m = 0.0;
    size_t i = 0;
    for (int l = t.levels; l >= 1; --l) {
        const size_t at = i * (size_t)adc::kPerRadix + (size_t)lane;
        const double v = l == 1 ? (double)t.leaf[at] : t.node[l - 1][at];
        const double c = per_scan(v, lane);
        if (l == t.levels) m = u53 * __shfl(c, 63, 64);
        const unsigned long long over = __ballot(c > m);
        int child;
        if (over) child = __ffsll(over) - 1;
        else {
            const unsigned long long nz = __ballot(v != 0.0);
            child = nz ? 63 - __clzll(nz) : 0;
        }
        const double before = __shfl(c, child > 0 ? child - 1 : 0, 64);
        if (child > 0) m = m - before;
        i = i * (size_t)adc::kPerRadix + (size_t)child;
        if (i >= (size_t)t.n[l - 1]) i = (size_t)t.n[l - 1] - 1;      // (the law's guard: never a padding node)
    }
    // (the law's guard: the scan's lanes round differently, and the slot stays inside the stored range whatever the leaves hold)
    if (size > 0 && i >= (size_t)size) i = (size_t)size - 1;
    if (lane == 0) {
        t.slot[b] = (int32_t)i;
        t.leaf_b[b] = t.leaf[i];
    }
}

// the batch's smallest sampled leaf, then every element's weight.  One workgroup per member
__global__ __launch_bounds__(256) void k_per_weights(PerView tv, float beta)
{
    __shared__ float red[4];
    const PerView t = per_member(tv, blockIdx.y);
    const int tid = threadIdx.x, B = t.B;
    float lo = __builtin_inff();
    for (int b = tid; b < B; b += 256) { const float x = t.leaf_b[b]; lo = x < lo ? x : lo; }
    for (int s = 32; s >= 1; s >>= 1) { const float x = __shfl_xor(lo, s, 64); lo = x < lo ? x : lo; }
    if ((tid & 63) == 0) red[tid >> 6] = lo;
    __syncthreads();
    lo = red[0];
    for (int k = 1; k < 4; ++k) lo = red[k] < lo ? red[k] : lo;
    for (int b = tid; b < B; b += 256) t.w[b] = adc::per_weight(lo, t.leaf_b[b], beta);
}

// pa(p_b) of every element from the critics' errors, and top = max(top, all of them).  One workgroup per member
__global__ __launch_bounds__(256) void k_per_priorities(PerView tv, adc::PerLaw law)
{
    __shared__ float red[4];
    const PerView t = per_member(tv, blockIdx.y);
    const int tid = threadIdx.x, B = t.B;
    float hi = 0.0f;
    for (int b = tid; b < B; b += 256) {
        const float pa = adc::per_pa(adc::per_priority(t.absd[2 * b], t.absd[2 * b + 1], law.eps, law.cap), law.alpha);
        t.pab[b] = pa;
        hi = pa > hi ? pa : hi;
    }
    for (int s = 32; s >= 1; s >>= 1) { const float x = __shfl_xor(hi, s, 64); hi = x > hi ? x : hi; }
    if ((tid & 63) == 0) red[tid >> 6] = hi;
    __syncthreads();
    if (tid == 0) {
        float top = t.top[0];
        for (int k = 0; k < 4; ++k) top = red[k] > top ? red[k] : top;
        t.top[0] = top;
    }
}

// the new leaf of every sampled slot: the largest pa(p) among the elements that drew it (duplicates write the same value)
// The batch passes through LDS a tile at a time: every lane reads the same entry, a broadcast
__global__ __launch_bounds__(256) void k_per_leaves(PerView tv)
{
    constexpr int kTile = 1024;
    __shared__ int32_t s_slot[kTile];
    __shared__ float s_pa[kTile];
    const PerView t = per_member(tv, blockIdx.y);
    const int tid = threadIdx.x, b = blockIdx.x * 256 + tid, B = t.B;
    const bool on = b < B;
    const int32_t s = on ? t.slot[b] : -1;
    float hi = on ? t.pab[b] : 0.0f;
    for (int o0 = 0; o0 < B; o0 += kTile) {
        const int cnt = B - o0 < kTile ? B - o0 : kTile;
        __syncthreads();
        for (int i = tid; i < cnt; i += 256) { s_slot[i] = t.slot[o0 + i]; s_pa[i] = t.pab[o0 + i]; }
        __syncthreads();
        for (int i = 0; i < cnt; ++i) {
            const float x = s_pa[i];
            if (s_slot[i] == s && x > hi) hi = x;
        }
    }
    if (on) t.leaf[s] = hi;
}

// node (slot[item] >> 6 level with by_slot, else first + item) of `level` from its children, a wave per item
__global__ __launch_bounds__(256) void k_per_rebuild(PerView tv, int level, int by_slot, long long first, long long items)
{
    const PerView t = per_member(tv, blockIdx.y);
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= items) return;
    const size_t node = by_slot ? (size_t)t.slot[item] >> (6 * level) : (size_t)(first + item);
    const size_t at = node * (size_t)adc::kPerRadix + (size_t)lane;
    const double v = level == 1 ? (double)t.leaf[at] : t.node[level - 1][at];
    const double c = per_scan(v, lane);
    if (lane == 63) t.node[level][node] = c;
}

// leaf = top over the slots [lo, lo + n): what a store or a buffer load wrote
__global__ void k_per_fill(PerView tv, long long lo, long long n)
{
    const PerView t = per_member(tv, blockIdx.y);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) t.leaf[lo + i] = t.top[0];
}

// the leaves after the ring's size changed under them: a stored slot without a leaf gets top, a slot past the size 0
__global__ void k_per_resize(PerView tv, long long size)
{
    const PerView t = per_member(tv, blockIdx.y);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n[0]) return;
    if (i >= size) t.leaf[i] = 0.0f;
    else if (t.leaf[i] == 0.0f) t.leaf[i] = t.top[0];
}

// every pair's donor's leaves, nodes and top into its destination's (adc_engine_pbt_exploit with rings; a member copy is one pair)
__global__ __launch_bounds__(256) void k_per_copy_pairs(PerView tv, const PbtPair *__restrict__ pairs)
{
    const PbtPair pr = pairs[blockIdx.y];
    const PerView s = per_member(tv, (size_t)pr.src), d = per_member(tv, (size_t)pr.dst);
    const size_t i0 = (size_t)blockIdx.x * 256u + threadIdx.x, step = (size_t)gridDim.x * 256u;
    for (size_t i = i0; i < tv.stride[0]; i += step) d.leaf[i] = s.leaf[i];
    for (int l = 1; l <= tv.levels; ++l)
        for (size_t i = i0; i < tv.stride[l]; i += step) d.node[l][i] = s.node[l][i];
    if (i0 == 0) d.top[0] = s.top[0];
}
