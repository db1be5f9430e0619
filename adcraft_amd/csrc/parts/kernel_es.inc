// kernel_es.inc - policy populations and the evolution strategy on the device: the flat parameter order against the policy
// kernel's chain-major layers, the members' perturbation, the per-env return of a generation, and the gradient estimate with
// its Adam / SGD step.  The arithmetic is adc_es.h's law, the code the host twins adc_es_noise_host / adc_es_update_host run.
// (part of the single translation unit adc_engine.hip)
// -------------------------------------------------------------------------------------------------
// Shape.  A lane owns four consecutive flat parameters - one Philox call per pair gives their four normals - and a workgroup
// 1024 of them.  k_es_perturb runs one such lane per (quad, pair) and writes both members of the pair; k_es_update regenerates
// the noise instead of reading it back and adds each parameter's terms in ascending pair order (the law's summation order,
// whatever the launch shape).  All stores are plain vector stores; nothing here is read by a step kernel.
// (a "layer" here is a term of the flat order: a recurrent policy's Wi | bi and Wh | bh stand among them as two more, adc_gru.h)
struct ParamLayout {
    int layers, P;                              // policy layers; flat length
    int n_in[adc::kMlpMaxTerms], n_out[adc::kMlpMaxTerms];
    int flat0[adc::kMlpMaxTerms];               // flat index of layer l's W[0][0] (its b[0] follows the weights)
    uint32_t offW[adc::kMlpMaxTerms], offb[adc::kMlpMaxTerms];      // floats from a member's base to its layer l (multiples of 4)
    uint32_t stride;                            // floats of a member's block
};

// one policy's layers: the centre's own allocations, or a member's (base + offW / offb)
struct ParamStore {
    float *W[adc::kMlpMaxTerms];
    float *b[adc::kMlpMaxTerms];
};

constexpr int kEsBlock = 256;

// flat parameter p: its layer, and its index inside that layer's weights (chain-major) or - bias - its biases
__device__ __forceinline__ void param_locate(const ParamLayout &L, int p, int &layer, bool &bias, uint32_t &idx)
{
    int l = 0;
    while (l + 1 < L.layers && p >= L.flat0[l + 1]) ++l;
    const int r = p - L.flat0[l], n_out = L.n_out[l], nw = L.n_in[l] * n_out;
    layer = l;
    bias = r >= nw;
    idx = bias ? (uint32_t)(r - nw) : (uint32_t)adc::mlp_weight_index(r / n_out, r % n_out, n_out);
}

// to_flat: flat[p] = the store's parameter p; else the store's parameter p = flat[p]
__global__ __launch_bounds__(kEsBlock) void k_params_copy(ParamLayout L, ParamStore s, float *__restrict__ flat, int to_flat)
{
    const int p = blockIdx.x * kEsBlock + threadIdx.x;
    if (p >= L.P) return;
    int l; bool bias; uint32_t idx;
    param_locate(L, p, l, bias, idx);
    float *slot = (bias ? s.b[l] : s.W[l]) + idx;
    if (to_flat) flat[p] = *slot;
    else *slot = flat[p];
}

// members 2i and 2i + 1 of pair i = blockIdx.y from the flat centre: theta + sigma * (+-eps) (noise != 0), or theta itself
__global__ __launch_bounds__(kEsBlock) void k_es_perturb(ParamLayout L, const float *__restrict__ theta, float *__restrict__ pop, size_t stride,
                                                         int M, int noise, uint64_t key, uint32_t generation, float sigma)
{
    const int q = blockIdx.x * kEsBlock + threadIdx.x, pair = blockIdx.y;
    if (4 * q >= L.P) return;
    float eps[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (noise) adc::es_noise4(key, (uint32_t)q, (uint32_t)pair, generation, eps);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = 4 * q + k;
        if (p >= L.P) break;
        int l; bool bias; uint32_t idx;
        param_locate(L, p, l, bias, idx);
        const size_t slot = (size_t)(bias ? L.offb[l] : L.offW[l]) + idx;
        const float t = theta[p];
#pragma unroll
        for (int sign = 0; sign < 2; ++sign) {
            const int member = 2 * pair + sign;
            if (member < M) pop[(size_t)member * stride + slot] = noise ? adc::es_perturbed(t, sigma, eps[k], sign) : t;
        }
    }
}

// the generation's return of every env: the step's float64 reward added behind the step, group by group in a chain
__global__ void k_es_accumulate(View v, double *__restrict__ es_return)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= v.N) return;
    es_return[env] = es_return[env] + v.reward[env];
}

// the gradient estimate from the shaped pair differences du[i] = u[2i] - u[2i + 1], the optimiser's step, and the centre's
// chain-major copy rebuilt from the new theta.  A workgroup owns 16 quads (64 parameters): sixteen lanes per quad regenerate the
// noise of sixteen pairs at a time and leave the products du[i] * eps in LDS; one lane per parameter then adds them in pair
// order - the law's sum, term for term - so the serial part of a parameter is its float64 additions, not its Philox calls
// (one lane per quad walking all pairs measured 240 us at 20 485 parameters x 256 pairs: 21 workgroups of dependent calls).
constexpr int kEsUpdQuads = 16, kEsUpdPairs = kEsBlock / kEsUpdQuads;
__global__ __launch_bounds__(kEsBlock) void k_es_update(ParamLayout L, ParamStore centre, float *__restrict__ theta, float *__restrict__ mom_m,
                                                        float *__restrict__ mom_v, float *__restrict__ grad, const double *__restrict__ du,
                                                        int M, uint64_t key, uint32_t generation, float sigma, adc::EsStep step)
{
    __shared__ double prod[kEsUpdPairs][kEsUpdQuads * 4];
    const int tid = threadIdx.x, ql = tid / kEsUpdPairs, sub = tid % kEsUpdPairs;
    const int q = blockIdx.x * kEsUpdQuads + ql;
    const bool quad_on = 4 * q < L.P;
    const int pairs = M >> 1;
    double acc = 0.0;                           // (lanes tid < 64: the sum of parameter blockIdx.x * 64 + tid)
    for (int base = 0; base < pairs; base += kEsUpdPairs) {
        const int i = base + sub;
        if (quad_on && i < pairs) {
            float eps[4];
            adc::es_noise4(key, (uint32_t)q, (uint32_t)i, generation, eps);
            const double d = du[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) prod[sub][ql * 4 + k] = adc::es_grad_term(d, eps[k]);
        }
        __syncthreads();
        if (tid < kEsUpdQuads * 4) {
            const int n = pairs - base < kEsUpdPairs ? pairs - base : kEsUpdPairs;
            for (int s = 0; s < n; ++s) acc = acc + prod[s][tid];
        }
        __syncthreads();
    }
    const int p = blockIdx.x * (kEsUpdQuads * 4) + tid;
    if (tid >= kEsUpdQuads * 4 || p >= L.P) return;
    const float t0 = theta[p];
    const float g = adc::es_decay(adc::es_grad_finish(acc, M, sigma), t0, step.l2);
    float m = mom_m[p], v = mom_v[p];
    const float t1 = adc::es_apply(step, t0, g, m, v);
    theta[p] = t1;
    mom_m[p] = m;
    mom_v[p] = v;
    grad[p] = g;
    int l; bool bias; uint32_t idx;
    param_locate(L, p, l, bias, idx);
    (bias ? centre.b[l] : centre.W[l])[idx] = t1;
}
