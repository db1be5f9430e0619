// kernel_pg.inc - policy-gradient training on the device: advantages from the rollout record, the forward recompute and the
// backward pass of the policy and value networks per sample, the weight gradient over samples, the statistics' sums and the
// optimiser step that rebuilds the policy kernel's chain-major layers.  The arithmetic is adc_pg.h's law, the code the host
// twins adc_pg_gae_host / adc_pg_grad_host / adc_pg_step_host run.
// (part of the single translation unit adc_engine.hip)
// -------------------------------------------------------------------------------------------------
// Shape.  k_pg_sample is k_mlp_policy's shape run both ways: one workgroup of 256 lanes per sample, every layer's activations
// in LDS, eight adjacent lanes per neuron with the butterfly join; the transposed pass reads the same chain-major weights with
// the roles of j and h swapped (a neuron's eight lanes read eight outputs' weights, 128 bytes apart - the layers are a few
// hundred KB and stay in L2).  It leaves every layer's input activations and deltas in a scratch buffer.  k_pg_wgrad then is
// X^T . Delta over samples in the law's chunk order: a workgroup owns a 16 x 16 tile of one layer's parameters (its bias the
// row j = n_in with x = 1) and ONE chunk of 1024 samples, stages 64 samples' 16 inputs and 16 deltas in LDS at a time, and every
// lane carries its parameter's float64 chain - one fused multiply-add per sample, exact products - and writes the chunk's
// partial; k_pg_grad_join adds a parameter's partials in chunk order.  No atomics; all stores are plain vector stores.
//
// Learner populations (adc_engine_pg_pop_*).  Every kernel has a k_pg_pop_* twin whose launch covers all M members: the member is
// one more grid dimension, what is a member's own (its layers, its loss constants, its step) is read from the device tables
// MlpLearner[M] / PgMember[M], and the member's samples, scratch rows, partials and parameters are the solo kernel's with a base
// moved to the member's block.  The bodies are shared (pg_sample_body, pg_wgrad_body, ...): a member runs the solo code on its own
// envs [m n, (m + 1) n) in its own order, so its bits are a solo engine's, whatever M and the other members are.
struct PgView {
    adc::PgShape sh;
    adc::PgLoss loss;
    MlpNet net[2];                          // the device's chain-major layers: [0] policy, [1] value
    const float *log_std;                   // [A] (free head)
    const float *obs, *action, *logp, *value;       // the record: [T][N][D], [T][N][A], [T][N], [T][N]
    const float *adv, *ret;                 // [T][N]
    int N, n0, B;                           // the engine's envs; the minibatch's first env and env count
    float *acts, *deltas, *pieces;          // scratch [S][na], [S][nd], [S][kPgPieces]
    int na, nd;
    int maxw;                               // the widest layer output of either network
};

// the KL penalty / value-clip add-on's side of a sample (adc_pg_kl.h; parts/kernel_pg_kl.inc): the snapshot of the collecting
// distribution and the add-on's own pieces
struct PgKlView {
    const float *mean_old;                  // [T][N][A]
    const float *ls_old;                    // [T][N][A] (two heads) or the clamped log_std vector(s) [A] / [M][A] (free head)
    int ls_per_sample;
    float *pieces;                          // scratch [S][kPgKlPieces]
};

// one term of the gradient: a layer's weights and bias, or log_std's row (n_in = 0)
struct PgTerm {
    const float *X;                         // the layer's input: the record's obs rows (obs != 0) or the scratch activations
    size_t ldx;
    int n_in, n_out, d_off, flat0, obs;
};

// the flat order against the device's stores (the terms in flat order)
struct PgLayout {
    int nterms, Q;
    int flat0[adc::kPgMaxTerms], n_in[adc::kPgMaxTerms], n_out[adc::kPgMaxTerms];
    float *W[adc::kPgMaxTerms], *b[adc::kPgMaxTerms];
};

// what is a member's own in a learner population, indexed by member on the device (its layers are MlpLearner's)
struct PgMember {
    adc::PgLoss loss;
    float gamma, gl, reward_scale;          // GAE; gl = gamma * lambda (the host's float32 product, as the solo launch gets it)
    int normalize;
    double mean, sd;                        // the advantage normalisation's moments (set between its passes)
    int clip;                               // the next update: clip on / off, the clip scale, the step's constants
    float scale;
    adc::EsStep step;
    int stopped;                            // shuffled minibatches: the member's update has stopped (k_pg_pop_update_live passes it by)
};

constexpr int kPgBlock = 256;

// (kl: the add-on's instantiation keeps the sample's mean_old / ls_old rows as well)
__host__ __device__ inline size_t pg_lds_floats(const adc::PgShape &sh, int maxw, bool kl = false)
{
    size_t n = (size_t)sh.D + 2u * (size_t)maxw + (kl ? 5u : 3u) * (size_t)sh.A;
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l < sh.layers[net]; ++l) n += (size_t)sh.n_out[net][l];
    return n;
}

__device__ __forceinline__ float *pg_param_slot(const PgLayout &L, int p)
{
    int i = 0;
    while (i + 1 < L.nterms && p >= L.flat0[i + 1]) ++i;
    const int r = p - L.flat0[i], n_out = L.n_out[i], nw = L.n_in[i] * n_out;
    return r >= nw ? L.b[i] + (r - nw) : L.W[i] + adc::mlp_weight_index(r / n_out, r % n_out, n_out);
}

// to_flat: flat[p] = the stores' parameter p; else the stores' parameter p = flat[p]
__global__ __launch_bounds__(kPgBlock) void k_pg_params_copy(PgLayout L, float *__restrict__ flat, int to_flat)
{
    const int p = blockIdx.x * kPgBlock + threadIdx.x;
    if (p >= L.Q) return;
    float *slot = pg_param_slot(L, p);
    if (to_flat) flat[p] = *slot;
    else *slot = flat[p];
}
// the same for the members member0 + blockIdx.y of a learner population: L is member 0's stores, a member's are `stride` floats
// further each; the member's flat vector is flat + blockIdx.y * flat_stride (flat_stride 0: one vector for all of them)
__global__ __launch_bounds__(kPgBlock) void k_pg_pop_params_copy(PgLayout L, size_t stride, int member0, float *__restrict__ flat, size_t flat_stride,
                                                                 int to_flat)
{
    const int p = blockIdx.x * kPgBlock + threadIdx.x;
    if (p >= L.Q) return;
    float *slot = pg_param_slot(L, p) + (size_t)(member0 + (int)blockIdx.y) * stride;
    float *f = flat + (size_t)blockIdx.y * flat_stride + p;
    if (to_flat) *f = *slot;
    else *slot = *f;
}

// one lane per env, walking the record backwards
__global__ void k_pg_gae(int N, int T, const float *__restrict__ reward, const uint8_t *__restrict__ term, const uint8_t *__restrict__ trunc,
                         const float *__restrict__ value, const float *__restrict__ boot, float gamma, float gl, float reward_scale,
                         float *__restrict__ adv_out, float *__restrict__ ret_out)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N) return;
    float adv = 0.0f, next = boot[env];
    for (int t = T - 1; t >= 0; --t) {
        const size_t i = (size_t)t * (size_t)N + (size_t)env;
        const float v = value[i];
        const float a = adc::pg_gae_day(reward[i], reward_scale, term[i] | trunc[i], v, next, gamma, gl, adv);
        adv_out[i] = a;
        ret_out[i] = a + v;
        next = v;
    }
}

// ... with the env's member's gamma, gamma * lambda and reward_scale (envs_per_member envs each, in env order)
__global__ void k_pg_pop_gae(int N, int T, int envs_per_member, const PgMember *__restrict__ mem, const float *__restrict__ reward,
                             const uint8_t *__restrict__ term, const uint8_t *__restrict__ trunc, const float *__restrict__ value,
                             const float *__restrict__ boot, float *__restrict__ adv_out, float *__restrict__ ret_out)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N) return;
    const PgMember &c = mem[env / envs_per_member];
    const float gamma = c.gamma, gl = c.gl, reward_scale = c.reward_scale;
    float adv = 0.0f, next = boot[env];
    for (int t = T - 1; t >= 0; --t) {
        const size_t i = (size_t)t * (size_t)N + (size_t)env;
        const float v = value[i];
        const float a = adc::pg_gae_day(reward[i], reward_scale, term[i] | trunc[i], v, next, gamma, gl, adv);
        adv_out[i] = a;
        ret_out[i] = a + v;
        next = v;
    }
}

// a chunk's partial of the law's chunked sum, one lane per (chunk, column): src[i * stride + col], i in the chunk.
// mode 0: f64(x);  1: (f64(x) - mean)^2, the square rounded;  2: f64(x) * f64(x), exact
__global__ void k_pg_chunk_sums(const float *__restrict__ src, long long n, int stride, int cols, int mode, double mean, double *__restrict__ part)
{
    const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long chunks = (n + adc::kPgChunk - 1) / adc::kPgChunk;
    if (lane >= chunks * cols) return;
    const long long chunk = lane / cols;
    const int col = (int)(lane % cols);
    const long long i0 = chunk * adc::kPgChunk, i1 = i0 + adc::kPgChunk < n ? i0 + adc::kPgChunk : n;
    double acc = 0.0;
    for (long long i = i0; i < i1; ++i) {
        const float x = src[(size_t)i * (size_t)stride + (size_t)col];
        acc = mode == 0 ? acc + (double)x : mode == 1 ? adc::pg_chain_sqdev(acc, x, mean) : adc::pg_chain_mac(acc, x, x);
    }
    part[lane] = acc;
}
// ... and the partials joined in chunk order, one lane per column
__global__ void k_pg_join(const double *__restrict__ part, long long chunks, int cols, double *__restrict__ out)
{
    const int col = threadIdx.x;
    if (col >= cols) return;
    double total = 0.0;
    for (long long c = 0; c < chunks; ++c) total = total + part[c * cols + col];
    out[col] = total;
}

__global__ void k_pg_normalize(float *__restrict__ adv, long long n, double mean, double std)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) adv[i] = adc::pg_normalized(adv[i], mean, std);
}

// the chunked sums of every member at once (blockIdx.y = member): term i < n of the member is row
// member * mstep + (inner ? (i / inner) * outer + i % inner : i) of src - the member's own order, whatever lies between its rows
// (inner = its envs, outer = N for the [T][N] advantages: i = t * n + local env).  mode as k_pg_chunk_sums, the mean the member's.
__global__ void k_pg_pop_chunk_sums(const float *__restrict__ src, int n, int inner, int outer, size_t mstep, int stride, int cols, int mode,
                                    const PgMember *__restrict__ mem, double *__restrict__ part, size_t part_stride)
{
    const int lane = blockIdx.x * blockDim.x + threadIdx.x, member = blockIdx.y;
    const int chunks = (n + adc::kPgChunk - 1) / adc::kPgChunk;
    if (lane >= chunks * cols) return;
    const int chunk = lane / cols, col = lane % cols;
    const int i0 = chunk * adc::kPgChunk, i1 = i0 + adc::kPgChunk < n ? i0 + adc::kPgChunk : n;
    const double mean = mode == 1 ? mem[member].mean : 0.0;
    const size_t base = (size_t)member * mstep;
    double acc = 0.0;
    for (int i = i0; i < i1; ++i) {
        const size_t row = base + (inner ? (size_t)(i / inner) * (size_t)outer + (size_t)(i % inner) : (size_t)i);
        const float x = src[row * (size_t)stride + (size_t)col];
        acc = mode == 0 ? acc + (double)x : mode == 1 ? adc::pg_chain_sqdev(acc, x, mean) : adc::pg_chain_mac(acc, x, x);
    }
    part[(size_t)member * part_stride + (size_t)lane] = acc;
}
// ... joined in chunk order, one workgroup per member, one lane per column: out[member * out_stride + col]
__global__ void k_pg_pop_join(const double *__restrict__ part, size_t part_stride, int chunks, int cols, double *__restrict__ out, int out_stride)
{
    const int col = threadIdx.x, member = blockIdx.x;
    if (col >= cols) return;
    const double *mine = part + (size_t)member * part_stride;
    double total = 0.0;
    for (int c = 0; c < chunks; ++c) total = total + mine[(size_t)c * cols + col];
    out[(size_t)member * out_stride + col] = total;
}

// one lane per recorded sample t * N + env; the env's member's moments, members that do not normalise left as they are
__global__ void k_pg_pop_normalize(float *__restrict__ adv, long long n, int N, int envs_per_member, const PgMember *__restrict__ mem)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PgMember &c = mem[(int)(i % N) / envs_per_member];
    if (c.normalize) adv[i] = adc::pg_normalized(adv[i], c.mean, c.sd);
}

// the transposed pass of one layer: dnew[j] = act'(y[j]) * sum8(n_out, h -> W[j][h] * dcur[h]) for the n inputs of the layer
__device__ __forceinline__ void pg_layer_back(const float *__restrict__ W, int n, int n_out, const float *y, const float *dcur, float *dnew,
                                              int activation, float *__restrict__ g_out)
{
    const int tid = threadIdx.x;
    const int pairs = n * adc::kMlpChains;
    for (int p0 = 0; p0 < pairs; p0 += kPgBlock) {
        const int pi = p0 + tid;
        const bool on = pi < pairs;
        const int j = on ? pi >> 3 : 0, c = pi & 7;
        float acc = 0.0f;
        if (on)
            for (int h = c; h < n_out; h += adc::kMlpChains) acc = adc::mlp_mac(acc, W[adc::mlp_weight_index(j, h, n_out)], dcur[h]);
        float s = acc;
        s = s + __shfl_xor(s, 1, 64);
        s = s + __shfl_xor(s, 2, 64);
        s = s + __shfl_xor(s, 4, 64);           // adc::mlp_join8
        if (on && c == 0) {
            const float d = adc::pg_hidden_delta(y[j], s, activation);
            dnew[j] = d;
            g_out[j] = d;
        }
    }
    __syncthreads();
}

// forward, head, loss and backward of sample s = t * B + (env - n0) with the layers `nets`, log_std and the loss constants given;
// the sample's scratch rows are row `slot` of p.acts / p.deltas / p.pieces.  kKl: with adc_pg_kl.h's KL penalty and value-loss clip
// (k, kl; ls_old_at: where the member's vector starts in k.ls_old with the free head) - the instantiation without is the code
// it was before there was one.  kGather: the sample's record row is grows[s] (adc_pg_shuffle.h; parts/kernel_pg_shuffle.inc),
// n0 and p.B are not read - again the instantiations without are the code they were.  kIm: the imitation loss of a teacher sample
// (adc_imitation.h; parts/kernel_imitation.inc) in the surrogate's place, logp and the weight where the KL's and the clip's pieces
// are - once more the instantiations without are the code they were
template <bool kKl, bool kGather = false, bool kIm = false>
__device__ __forceinline__ void pg_sample_body(const PgView &p, const MlpNet *nets, const float *log_std, const adc::PgLoss &loss, int n0, size_t s,
                                               size_t slot, const PgKlView &k, const adc::PgKl &kl, size_t ls_old_at,
                                               const uint32_t *__restrict__ grows = nullptr, const adc::ImLaw &im = adc::ImLaw{})
{
    extern __shared__ __align__(16) float pg_lds[];
    __shared__ float s_g, s_dv;
    const adc::PgShape &sh = p.sh;
    const int tid = threadIdx.x, A = sh.A, D = sh.D;
    size_t row;
    if constexpr (kGather) row = (size_t)grows[s];
    else row = (s / (size_t)p.B) * (size_t)p.N + (size_t)n0 + s % (size_t)p.B;
    float *x = pg_lds, *ybase = x + D;
    float *y[2][adc::kMlpMaxLayers];
    {
        float *q = ybase;
        for (int net = 0; net < 2; ++net)
            for (int l = 0; l < sh.layers[net]; ++l) { y[net][l] = q; q += sh.n_out[net][l]; }
        ybase = q;
    }
    float *d0 = ybase, *d1 = d0 + p.maxw, *zs = d1 + p.maxw, *sds = zs + A, *lss = sds + A;
    float *mos = lss + A, *los = mos + A;   // (kKl only: the LDS region ends at lss + A otherwise)
    for (int j = tid; j < D; j += kPgBlock) x[j] = p.obs[row * (size_t)D + j];
    __syncthreads();
    float *acts = p.acts + slot * (size_t)p.na, *deltas = p.deltas + slot * (size_t)p.nd;
    // forward, every layer's activations kept (and the hidden ones written out for the weight gradient)
    {
        int ao = 0;
        for (int net = 0; net < 2; ++net) {
            const float *in = x;
            for (int l = 0; l < sh.layers[net]; ++l) {
                const bool last = l + 1 == sh.layers[net];
                const int n_out = sh.n_out[net][l];
                mlp_layer(nets[net].W[l], nets[net].b[l], adc::pg_n_in(sh, net, l), n_out, in, y[net][l], last ? -1 : sh.activation);
                if (!last) {
                    for (int h = tid; h < n_out; h += kPgBlock) acts[ao + h] = y[net][l][h];
                    ao += n_out;
                }
                in = y[net][l];
            }
        }
    }
    // head: z, sd, ls of every component; the log-probability's terms in d0
    const float *o = y[0][sh.layers[0] - 1];
    for (int a = tid; a < A; a += kPgBlock) {
        const float raw = sh.two_heads ? o[A + a] : log_std[a];
        const float ls = adc::mlp_clamp_log_std(raw, sh.clamp, sh.ls_lo, sh.ls_hi);
        const float sd = adc::mlp_exp(ls);
        const float z = adc::pg_z(p.action[row * (size_t)A + a], o[a], sd);
        zs[a] = z; sds[a] = sd; lss[a] = ls;
        d0[a] = adc::mlp_logp_term(z, ls);
        if constexpr (kKl) {     // the collecting distribution's row, and the KL's terms in d1
            const float mo = k.mean_old[row * (size_t)A + a];
            const float lo = k.ls_per_sample ? k.ls_old[row * (size_t)A + a] : k.ls_old[ls_old_at + a];
            mos[a] = mo; los[a] = lo;
            d1[a] = adc::pg_kl_term(o[a], ls, sd, mo, lo, adc::mlp_exp(lo));
        }
    }
    __syncthreads();
    if (tid < kWave) {       // the first eight lanes: the chains of the two (kKl: three) sum8 over the components
        const int c = tid & 7;
        float st = 0.0f, sl = 0.0f, sk = 0.0f;
        if (tid < adc::kMlpChains)
            for (int a = c; a < A; a += adc::kMlpChains) {
                st = st + d0[a]; sl = sl + lss[a];
                if constexpr (kKl) sk = sk + d1[a];
            }
        st = st + __shfl_xor(st, 1, 64); sl = sl + __shfl_xor(sl, 1, 64);
        st = st + __shfl_xor(st, 2, 64); sl = sl + __shfl_xor(sl, 2, 64);
        st = st + __shfl_xor(st, 4, 64); sl = sl + __shfl_xor(sl, 4, 64);
        if constexpr (kKl) {
            sk = sk + __shfl_xor(sk, 1, 64);
            sk = sk + __shfl_xor(sk, 2, 64);
            sk = sk + __shfl_xor(sk, 4, 64);
        }
        if (tid == 0) {
            const float logp = adc::mlp_logp_finish(st, A), entropy = adc::pg_entropy_finish(sl, A);
            const float logp_old = p.logp[row], ret = p.ret[row];
            float pol_loss, val_loss, g, w = 0.0f;
            int clipped = 0;
            if constexpr (kIm) {
                w = adc::im_weight(p.adv[row], im);
                g = adc::im_surrogate(w, logp, pol_loss);
            } else {
                const float ratio = adc::mlp_exp(logp - logp_old);
                g = adc::pg_surrogate(ratio, p.adv[row], loss.eps_clip, pol_loss, clipped);
            }
            const float V = sh.layers[1] ? y[1][sh.layers[1] - 1][0] : 0.0f;
            float dv;
            if constexpr (kKl) {
                int vf_clipped;
                dv = adc::pg_kl_dvalue(V, ret, loss.vf_coef, kl.vf_clip, val_loss, vf_clipped);
                float *pk = k.pieces + slot * (size_t)adc::kPgKlPieces;
                pk[adc::kPgKlKl] = sk; pk[adc::kPgKlVfClipped] = vf_clipped ? 1.0f : 0.0f;
            } else dv = adc::pg_dvalue(V, ret, loss.vf_coef, val_loss);
            s_g = g; s_dv = dv;
            float *pc = p.pieces + slot * (size_t)adc::kPgPieces;
            pc[adc::kPgPolLoss] = pol_loss; pc[adc::kPgValLoss] = val_loss; pc[adc::kPgEntropy] = entropy; pc[adc::kPgKl] = kIm ? logp : logp_old - logp;
            pc[adc::kPgClipped] = kIm ? w : clipped ? 1.0f : 0.0f; pc[adc::kPgRet] = ret; pc[adc::kPgErr] = ret - p.value[row]; pc[7] = 0.0f;
        }
    }
    __syncthreads();
    // where a network's deltas go in the sample's scratch row
    int doff[2][adc::kMlpMaxLayers], dfree = 0;
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l < sh.layers[net]; ++l) { doff[net][l] = dfree; dfree += sh.n_out[net][l]; }
    // the policy network's output deltas (means, then log-stds; the free vector's go to their own row), then its hidden layers'
    {
        const float g = s_g;
        const int L = sh.layers[0];
        float *gout = deltas + doff[0][L - 1];
        for (int a = tid; a < A; a += kPgBlock) {
            const float raw = sh.two_heads ? o[A + a] : log_std[a];
            const int moved = adc::pg_clamp_moved(raw, sh.clamp, sh.ls_lo, sh.ls_hi);
            float dm = adc::pg_dmean(g, zs[a], sds[a]);
            float dl = adc::pg_dls(g, zs[a], loss.ent_coef, moved);
            if constexpr (kIm)
                if (!im.train_log_std) dl = 0.0f;
            if constexpr (kKl)
                if (kl.coef != 0.0f) {          // (wave-uniform; a zero coefficient adds nothing: adc_pg.h's bits)
                    dm = adc::pg_kl_add(dm, kl.coef, adc::pg_kl_dmean(o[a], sds[a], mos[a]));
                    dl = adc::pg_kl_add(dl, kl.coef, adc::pg_kl_dls(o[a], sds[a], mos[a], adc::mlp_exp(los[a]), moved));
                }
            d0[a] = dm; gout[a] = dm;
            if (sh.two_heads) { d0[A + a] = dl; gout[A + a] = dl; }
            else deltas[dfree + a] = dl;
        }
        __syncthreads();
        float *dcur = d0, *dnew = d1;
        for (int l = L - 2; l >= 0; --l) {
            pg_layer_back(nets[0].W[l + 1], sh.n_out[0][l], sh.n_out[0][l + 1], y[0][l], dcur, dnew, sh.activation, deltas + doff[0][l]);
            float *t = dcur; dcur = dnew; dnew = t;
        }
    }
    if (sh.layers[1] > 0) {
        const int L = sh.layers[1];
        if (tid == 0) { d0[0] = s_dv; deltas[doff[1][L - 1]] = s_dv; }
        __syncthreads();
        float *dcur = d0, *dnew = d1;
        for (int l = L - 2; l >= 0; --l) {
            pg_layer_back(nets[1].W[l + 1], sh.n_out[1][l], sh.n_out[1][l + 1], y[1][l], dcur, dnew, sh.activation, deltas + doff[1][l]);
            float *t = dcur; dcur = dnew; dnew = t;
        }
    }
}

__global__ __launch_bounds__(kPgBlock) void k_pg_sample(PgView p)
{
    pg_sample_body<false>(p, p.net, p.log_std, p.loss, p.n0, blockIdx.x, blockIdx.x, PgKlView{}, adc::PgKl{}, 0);
}
// sample blockIdx.x of member blockIdx.y's minibatch: the member's layers and loss constants, its envs from member * envs_per_member
// on, its scratch rows from member * gridDim.x on (p.net, p.log_std and p.loss are not read)
__global__ __launch_bounds__(kPgBlock) void k_pg_pop_sample(PgView p, const MlpLearner *__restrict__ learners, const PgMember *__restrict__ mem,
                                                            int envs_per_member)
{
    const int member = blockIdx.y;
    pg_sample_body<false>(p, learners[member].net, learners[member].log_std, mem[member].loss, p.n0 + member * envs_per_member, blockIdx.x,
                          (size_t)member * gridDim.x + blockIdx.x, PgKlView{}, adc::PgKl{}, 0);
}

// one term's partials: gpart[chunk][flat0 + j * n_out + h] = the chunk's chain of x_s[j] * delta_s[h]; a 16 x 16 tile (blockIdx.x)
// and a chunk (blockIdx.y) per workgroup
constexpr int kPgTile = 16, kPgSlab = 64;
// (kGather: the observation term's record row of sample s is grows[s]; B, N and n0 are not read)
template <bool kGather = false>
__device__ __forceinline__ void pg_wgrad_body(const PgTerm &t, long long S, int B, int N, int n0, const float *__restrict__ deltas, int nd,
                                              double *__restrict__ gpart, int Q, const uint32_t *__restrict__ grows = nullptr)
{
    __shared__ float xs[kPgSlab][kPgTile + 1], ds[kPgSlab][kPgTile + 1];
    const int tid = threadIdx.x, jj = tid >> 4, hh = tid & 15;
    const int tiles_h = (t.n_out + kPgTile - 1) / kPgTile;
    const int j0 = ((int)blockIdx.x / tiles_h) * kPgTile, h0 = ((int)blockIdx.x % tiles_h) * kPgTile;
    const int jx = j0 + hh, hx = h0 + hh;       // (the column this lane stages)
    double part = 0.0;
    const long long c0 = (long long)blockIdx.y * adc::kPgChunk, c1 = c0 + adc::kPgChunk < S ? c0 + adc::kPgChunk : S;
    for (long long s0 = c0; s0 < c1; s0 += kPgSlab) {
        const int n = c1 - s0 < kPgSlab ? (int)(c1 - s0) : kPgSlab;
#pragma unroll
        for (int pass = 0; pass < kPgSlab / kPgTile; ++pass) {
            const int si = pass * kPgTile + jj;
            if (si < n) {
                const long long s = s0 + si;
                float xv = 1.0f;                // (the bias row j = n_in; rows beyond it are never stored)
                if (jx < t.n_in) {
                    size_t row;
                    if constexpr (kGather) row = t.obs ? (size_t)grows[s] : (size_t)s;
                    else {
                        const uint32_t su = (uint32_t)s, day = su / (uint32_t)B;      // (S < 2^31: 32-bit division)
                        row = t.obs ? (size_t)day * (size_t)N + (size_t)n0 + (size_t)(su - day * (uint32_t)B) : (size_t)s;
                    }
                    xv = t.X[row * t.ldx + (size_t)jx];
                }
                xs[si][hh] = xv;
                ds[si][hh] = hx < t.n_out ? deltas[(size_t)s * (size_t)nd + (size_t)(t.d_off + hx)] : 0.0f;
            }
        }
        __syncthreads();
        for (int i = 0; i < n; ++i) part = adc::pg_chain_mac(part, xs[i][jj], ds[i][hh]);
        __syncthreads();
    }
    const int j = j0 + jj, h = h0 + hh;
    if (j <= t.n_in && h < t.n_out) gpart[(size_t)blockIdx.y * (size_t)Q + (size_t)t.flat0 + (size_t)j * (size_t)t.n_out + (size_t)h] = part;
}
__global__ __launch_bounds__(kPgBlock) void k_pg_wgrad(PgTerm t, long long S, int B, int N, int n0, const float *__restrict__ deltas, int nd,
                                                       double *__restrict__ gpart, int Q)
{
    pg_wgrad_body(t, S, B, N, n0, deltas, nd, gpart, Q);
}
// member blockIdx.z's tile and chunk: its envs, its S scratch rows, its gridDim.y chunks of partials
__global__ __launch_bounds__(kPgBlock) void k_pg_pop_wgrad(PgTerm t, long long S, int B, int N, int n0, int envs_per_member,
                                                           const float *__restrict__ deltas, int nd, double *__restrict__ gpart, int Q)
{
    const size_t member = blockIdx.z, row0 = member * (size_t)S;
    if (!t.obs && t.X) t.X += row0 * t.ldx;
    pg_wgrad_body(t, S, B, N, n0 + (int)member * envs_per_member, deltas + row0 * (size_t)nd, nd, gpart + member * gridDim.y * (size_t)Q, Q);
}

// a parameter's partials joined in chunk order: grad[p] = float32(total / S)
__global__ __launch_bounds__(kPgBlock) void k_pg_grad_join(const double *__restrict__ gpart, int chunks, int Q, long long S, float *__restrict__ grad)
{
    const int p = blockIdx.x * kPgBlock + threadIdx.x;
    if (p >= Q) return;
    double total = 0.0;
    for (int c = 0; c < chunks; ++c) total = total + gpart[(size_t)c * (size_t)Q + (size_t)p];
    grad[p] = adc::pg_grad_finish(total, S);
}
// ... of every member (blockIdx.y): its `chunks` rows of partials, its row of grad
__global__ __launch_bounds__(kPgBlock) void k_pg_pop_grad_join(const double *__restrict__ gpart, int chunks, int Q, long long S, float *__restrict__ grad)
{
    const int p = blockIdx.x * kPgBlock + threadIdx.x;
    if (p >= Q) return;
    const double *mine = gpart + (size_t)blockIdx.y * (size_t)chunks * (size_t)Q;
    double total = 0.0;
    for (int c = 0; c < chunks; ++c) total = total + mine[(size_t)c * (size_t)Q + (size_t)p];
    grad[(size_t)blockIdx.y * (size_t)Q + (size_t)p] = adc::pg_grad_finish(total, S);
}

// the (clipped) gradient's step on theta, and the device's chain-major layers and log_std rebuilt from the new theta
__global__ __launch_bounds__(kPgBlock) void k_pg_update(PgLayout L, float *__restrict__ theta, float *__restrict__ mom_m, float *__restrict__ mom_v,
                                                        const float *__restrict__ grad, int clip, float scale, adc::EsStep step)
{
    const int p = blockIdx.x * kPgBlock + threadIdx.x;
    if (p >= L.Q) return;
    float g = grad[p];
    if (clip) g = g * scale;
    float m = mom_m[p], v = mom_v[p];
    const float t1 = adc::pg_apply(step, theta[p], g, m, v);
    theta[p] = t1;
    mom_m[p] = m;
    mom_v[p] = v;
    *pg_param_slot(L, p) = t1;
}
// ... of every member (blockIdx.y) with its own clip scale and step constants (the clip, scale and step of its Row: PgMember, or
// the off-policy populations' Td3PopStep; set by the host before the launch); theta, the moments and grad are [M][Q], L member 0's
// stores and a member's `stride` floats further each
template <class Row>
__device__ __forceinline__ void pg_pop_update_body(const PgLayout &L, size_t stride, float *__restrict__ theta, float *__restrict__ mom_m,
                                                   float *__restrict__ mom_v, const float *__restrict__ grad, const Row *__restrict__ mem)
{
    const int p = blockIdx.x * kPgBlock + threadIdx.x;
    if (p >= L.Q) return;
    const size_t member = blockIdx.y, i = member * (size_t)L.Q + (size_t)p;
    const Row &c = mem[member];
    float g = grad[i];
    if (c.clip) g = g * c.scale;
    float m = mom_m[i], v = mom_v[i];
    const float t1 = adc::pg_apply(c.step, theta[i], g, m, v);
    theta[i] = t1;
    mom_m[i] = m;
    mom_v[i] = v;
    *(pg_param_slot(L, p) + member * stride) = t1;
}
__global__ __launch_bounds__(kPgBlock) void k_pg_pop_update(PgLayout L, size_t stride, float *__restrict__ theta, float *__restrict__ mom_m,
                                                            float *__restrict__ mom_v, const float *__restrict__ grad,
                                                            const PgMember *__restrict__ mem)
{
    pg_pop_update_body(L, stride, theta, mom_m, mom_v, grad, mem);
}
