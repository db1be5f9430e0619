// kernel_mlp_policy.inc - the learned agent on the device: a fully connected policy network (and an optional value network)
// evaluated on the engine's own observation arrays, a diagonal Gaussian head sampled from the agent's Philox stream, cent bids
// and budgets into the engine's action buffers, and the rollout record a trainer reads.  The arithmetic is adc_mlp.h's law,
// the code the host twin adc_mlp_act_host runs too.
// (part of the single translation unit adc_engine.hip)
// -------------------------------------------------------------------------------------------------
// Shape.  One workgroup of 256 lanes per env; the env's input row and the activations live in LDS.  A layer is a loop over
// (neuron, chain) pairs: eight adjacent lanes own the eight chains of one neuron's sum (adc_mlp.h sum8) and join them by a
// butterfly, so a [., 32] layer keeps all 256 lanes busy; a lane's 16-byte load is its chain's next four weights, a wavefront's
// loads 1 KB in a row (adc::mlp_weight_index).  The kernel is bound by the latency of its dependent rounds of weight loads, not
// by their traffic: several envs per workgroup sharing each loaded weight were built and measured no faster at 4096 x 256 and
// slower at 16384 x 1024 (fewer resident workgroups), so there is one env per workgroup (profiles/pr_mlp_policy.txt).
struct MlpNet {
    const float *W[adc::kMlpMaxLayers];     // chain-major blocks of 32 inputs, adc::mlp_weight_index
    const float *b[adc::kMlpMaxLayers];
    int n_in[adc::kMlpMaxLayers], n_out[adc::kMlpMaxLayers];
    int layers;                             // 0: no such network
};

// one learner's own stores (adc_engine_mlp_learners): every layer chain-major as above
struct MlpLearner {
    MlpNet net[2];                          // [0] policy, [1] value
    const float *log_std;                   // [A] (free head; null with two heads)
};

struct MlpView {
    MlpNet pol, val;
    const float *shift, *scale;             // [D] or null: no normalisation
    size_t norm_stride;                     // floats between two learners' vectors (adc_engine_obs_norm_init, per_member); 0: shared
    const float *log_std;                   // [A] free parameter vector (head of A outputs)
    int activation, two_heads, clamp, deterministic;
    float ls_lo, ls_hi, clip_hi;
    int A, D, P;                            // action size K+1, input size frames * (5K+2), the policy network's outputs (A or 2A)
    uint64_t *key;                          // [N] the agent's own stream (stage ST_MLP)
    uint32_t *tick;                         // [N]
    float *mean, *ls, *action;              // [N][A] of the last act
    float *logp, *value;                    // [N]
    // a population (adc_engine_mlp_population): env -> member, and the members' policy layers at pop + member * pop_stride
    // (+ pop_offW[l] / pop_offb[l]), each layer in the layout of W / b above.  member == null: every env runs `pol`.
    // Learners (adc_engine_mlp_learners): env -> member as well, and `learners[member]` names the member's own policy layers,
    // value layers and log_std (pop_stride is 0 then: that is how the host tells the two kinds apart).
    const int32_t *member;                  // [N]
    union {
        const float *pop;
        const MlpLearner *learners;       // [M], on the device
    };
    size_t pop_stride;                      // floats
    uint32_t pop_offW[adc::kMlpMaxLayers], pop_offb[adc::kMlpMaxLayers];
    // the squashed action (adc_engine_mlp_set_squash; with learners adc_engine_mlp_learners_set_squash): the env is given
    // lo + half * (tanh(a) + 1).  null: off
    const float *sq_lo, *sq_half;           // [A]
    // the observation history (adc_engine_mlp_init_frames, frames > 1; adc_mlp.h): null / 1 without one
    float *hist;                            // [N][frames][5K+2] raw frames, slot = episode day mod frames
    int32_t *last, *from;                   // [N] the episode day of the last act (-2: none); the first day whose frame is valid
    int frames;
    // the bounded act (adc_engine_mlp_set_bounds; with learners adc_engine_mlp_learners_set_bounds; adc_mlp.h "bounded"): the action is
    // n in [-1, 1] and the env is given lo + half * (n + 1).  null: off.  explore: adc::kMlpGaussian or adc::kMlpRandom (read by the
    // bounded kernels alone)
    const float *bd_lo, *bd_half;           // [A]
    int explore;
};

// where one recorded day goes: the slot's rows of the view's first env (null: that field is off)
struct MlpRecordSlot {
    float *action;                          // [N][A]
    float *logp, *value;                    // [N]
    float *obs;                             // [N][D]
    int raw_obs;                            // the obs row is the flat observation before normalisation (adc_engine_td3_norm_init); 0: the network's input
};

constexpr int kMlpBlock = 256;

// floats of LDS: input row | two activation buffers | the policy network's outputs
__host__ __device__ inline size_t mlp_lds_floats(int D, int P) { return (size_t)D + 2u * adc::kMlpMaxWidth + (size_t)P; }

__device__ __forceinline__ void mlp_layer(const float *__restrict__ W, const float *__restrict__ b, int n_in, int n_out,
                                          const float *in, float *out, int activation)
{
    const int tid = threadIdx.x;
    const int pairs = n_out * adc::kMlpChains;
    for (int p0 = 0; p0 < pairs; p0 += kMlpBlock) {
        const int pi = p0 + tid;
        const bool on = pi < pairs;
        const int h = on ? pi >> 3 : 0, c = pi & 7;
        float acc = 0.0f;
        if (on) {
            // a 16-byte load = the chain's next four weights (adc::mlp_weight_index); whole blocks of 32 inputs first, then the tail
            const float4 *w4 = reinterpret_cast<const float4 *>(W) + ((size_t)h * 8u + (size_t)c);
            const size_t wstep = (size_t)n_out * 8u;
            const int full = n_in >> 5;
#pragma unroll 4
            for (int i = 0; i < full; ++i) {
                const float4 w = w4[(size_t)i * wstep];
                const float *x = in + ((i << 5) + c);
                acc = adc::mlp_mac(acc, w.x, x[0]);
                acc = adc::mlp_mac(acc, w.y, x[8]);
                acc = adc::mlp_mac(acc, w.z, x[16]);
                acc = adc::mlp_mac(acc, w.w, x[24]);
            }
            if (n_in & 31) {
                const float4 w = w4[(size_t)full * wstep];
                const float wq[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = (full << 5) + c + 8 * q;
                    if (j < n_in) acc = adc::mlp_mac(acc, wq[q], in[j]);
                }
            }
        }
        float s = acc;
        s = s + __shfl_xor(s, 1, 64);           // (s0 + s1), (s2 + s3), ...
        s = s + __shfl_xor(s, 2, 64);           // (s0 + s1) + (s2 + s3), ...
        s = s + __shfl_xor(s, 4, 64);           // adc::mlp_join8
        if (on && c == 0) {
            const float y = s + b[h];
            out[h] = activation >= 0 ? adc::mlp_act(y, activation) : y;
        }
    }
    __syncthreads();
}

// one network on the input row at `lds`; leaves its outputs at out_last.  kPop: the layers are a member's (at mbase), not net's own
template <bool kPop>
__device__ __forceinline__ void mlp_network(const MlpNet &net, const MlpView &p, const float *mbase, int activation, float *lds, int D,
                                            float *out_last)
{
    const float *in = lds;
    float *h0 = lds + D, *h1 = h0 + adc::kMlpMaxWidth;
    for (int l = 0; l < net.layers; ++l) {
        const bool last = l + 1 == net.layers;
        float *out = last ? out_last : ((l & 1) ? h1 : h0);
        const float *W = kPop ? mbase + p.pop_offW[l] : net.W[l];
        const float *b = kPop ? mbase + p.pop_offb[l] : net.b[l];
        mlp_layer(W, b, net.n_in[l], net.n_out[l], in, out, last ? -1 : activation);
        in = out;
    }
}

// Element i of the raw input row an act of `env` would read now: frame 0 from the engine's output arrays (zeros on the first day
// of an episode), with a history (kHist) frames 1 .. H-1 from the env's raw frames under `from` (adc::mlp_hist_from of the
// env's words: the caller reads them once).  The act and mode 1 of the kernels with a history and the trainers' store bodies
// all form their rows with it (the kernels without one keep the statements they had, which are its kHist = false case);
// consecutive i are consecutive floats of one frame, so a wavefront's loads are coalesced.
template <bool kHist>
__device__ __forceinline__ float mlp_row_raw_at(const View &v, const float *__restrict__ hist, int frames, int env, int i, bool first, double cum,
                                                int32_t days, int32_t d, int32_t from)
{
    const int K = v.K;
    const size_t o = (size_t)env * K;
    if constexpr (kHist) {
        const int D0 = 5 * K + 2;
        if (i >= D0) return adc::mlp_hist_at(i, D0, frames, hist + (size_t)env * (size_t)frames * (size_t)D0, d, from);
    }
    return first ? 0.0f : adc::mlp_obs_at(i, K, v.clk + o, v.cost + o, v.imp + o, v.rev + o, v.conv + o, cum, days);
}

// mode 0: act (policy and value networks, sample, actions, record);  mode 1: the value network alone into value_out (the
// bootstrap value of the observation the last step left) - no draw, no tick, nothing else written.
// kMembers 0: every env runs `pol`;  1: the env's policy layers are its member's (a population);  2: the policy layers, the
// value layers and log_std are the env's learner's.  (Three instantiations, so that the single-policy kernel and the
// population's are the code they were.)
// kSquash: the env is given the squashed action (adc::mlp_squash).  The single-policy kernel has that form
// (adc_engine_mlp_set_squash) and the learners' kernel has it (adc_engine_mlp_learners_set_squash: one pair of bounds for all
// members); without it the three kernels compute what they computed before there was one.
// kHist: the input row is the last `frames` raw observations (adc_mlp.h, observation history); mode 0 then writes this act's
// raw frame 0 and the env's two validity words, mode 1 writes none of them.  Without it the kernels are the code they were.
// kBounded: the bounded act (adc_mlp.h "bounded"; kMembers 0 and 2, never with kSquash): the action and the record hold n, the env is
// given its box image, logp is +0.  Without it the kernels are the code they were.
template <int kMembers, bool kSquash = false, bool kHist = false, bool kBounded = false>
__global__ __launch_bounds__(kMlpBlock) void k_mlp_policy(View v, MlpView p, int mode, const float *__restrict__ replay_z,
                                                          float budget_override, float *__restrict__ bids, float *__restrict__ budgets,
                                                          MlpRecordSlot rec, float *__restrict__ value_out)
{
    extern __shared__ __align__(16) float mlp_lds[];
    __shared__ float s_value;
    const int tid = threadIdx.x, K = v.K, D = p.D, A = p.A, env = blockIdx.x;
    // the input row: zeros on the first day of an episode (the reset observation), else the last step's outputs
    {
        // (without a history the loop below is, statement for statement, the code it was: the instantiations that existed before
        // the history keep their register allocation)
        const bool first = v.day[env] == 0;
        const int32_t d = kHist ? v.day[env] : 0;
        const size_t o = (size_t)env * K;
        const double cum = v.cum_profit[env];
        const int32_t days = v.day_out[env];
        int32_t from = 0;
        if constexpr (kHist) from = adc::mlp_hist_from(d, p.last[env], p.from[env]);
        // (learners may have a normaliser each: the env's member's row of the vectors; the stride is 0 whenever they are shared)
        const size_t no = kMembers == 2 ? (size_t)p.member[env] * p.norm_stride : 0;
        for (int j = tid; j < D; j += kMlpBlock) {
            float xj;
            if constexpr (kHist) xj = mlp_row_raw_at<true>(v, p.hist, p.frames, env, j, first, cum, days, d, from);
            else xj = first ? 0.0f : adc::mlp_obs_at(j, K, v.clk + o, v.cost + o, v.imp + o, v.rev + o, v.conv + o, cum, days);
            const float raw = xj;
            if (p.shift) xj = adc::mlp_normalize(xj, p.shift[no + j], p.scale[no + j]);
            mlp_lds[j] = xj;
            if (mode == 0 && rec.obs) rec.obs[(size_t)env * D + j] = rec.raw_obs ? raw : xj;
        }
        __syncthreads();
        if constexpr (kHist) {
            // every read of the history is behind the barrier: this act's raw frame 0 into slot d mod H, then the validity words
            if (mode == 0) {
                const int D0 = 5 * K + 2;
                float *slot = p.hist + ((size_t)env * (size_t)p.frames + (size_t)adc::mlp_hist_slot(d, p.frames)) * (size_t)D0;
                for (int j = tid; j < D0; j += kMlpBlock) slot[j] = mlp_row_raw_at<false>(v, nullptr, 1, env, j, first, cum, days, d, 0);
                if (tid == 0) { p.last[env] = d; p.from[env] = from; }
            }
        }
    }
    float *out = mlp_lds + D + 2 * adc::kMlpMaxWidth;
    const MlpLearner *lm = kMembers == 2 ? p.learners + p.member[env] : nullptr;
    if (p.val.layers > 0) {
        // (the value network's single output lands in the first float of `out`, which the policy network overwrites afterwards)
        if (kMembers == 2) mlp_network<false>(lm->net[1], p, nullptr, p.activation, mlp_lds, D, out);
        else mlp_network<false>(p.val, p, nullptr, p.activation, mlp_lds, D, out);
        if (tid == 0) s_value = out[0];
        __syncthreads();
    } else if (tid == 0) s_value = 0.0f;
    if (mode == 1) {
        if (tid == 0) value_out[env] = s_value;
        return;
    }
    if (kMembers == 2) mlp_network<false>(lm->net[0], p, nullptr, p.activation, mlp_lds, D, out);
    else mlp_network<kMembers == 1>(p.pol, p, kMembers == 1 ? p.pop + (size_t)p.member[env] * p.pop_stride : nullptr, p.activation, mlp_lds, D, out);
    // heads, sample, the env's action; the log-probability's terms replace the means in LDS
    const uint64_t key = p.key[env];
    const uint32_t tick = p.tick[env];
    for (int a = tid; a < A; a += kMlpBlock) {
        const float mean = out[a];
        const float ls = adc::mlp_clamp_log_std(p.two_heads ? out[A + a] : (kMembers == 2 ? lm->log_std : p.log_std)[a], p.clamp, p.ls_lo, p.ls_hi);
        float z = 0.0f;
        float act;
        if constexpr (kBounded) {
            uint32_t w = 0u;
            if (!p.deterministic) {
                if (p.explore == adc::kMlpRandom) w = adc::mlp_word(key, tick, a);
                else z = replay_z ? replay_z[(size_t)env * A + a] : adc::mlp_normal(key, tick, a);
            }
            act = adc::mlp_bounded_action(mean, ls, z, w, p.deterministic, p.explore);
        } else {
            if (!p.deterministic) z = replay_z ? replay_z[(size_t)env * A + a] : adc::mlp_normal(key, tick, a);
            act = adc::mlp_sample(mean, ls, z, p.deterministic);
        }
        const size_t oa = (size_t)env * A + a;
        p.mean[oa] = mean;
        p.ls[oa] = ls;
        p.action[oa] = act;
        if (rec.action) rec.action[oa] = act;
        float ea;
        if constexpr (kBounded) ea = adc::mlp_box(act, p.bd_lo[a], p.bd_half[a]);
        else ea = kSquash ? adc::mlp_squash(act, p.sq_lo[a], p.sq_half[a]) : act;
        if (a == 0) budgets[env] = adc::mlp_budget(ea, budget_override);
        else bids[(size_t)env * K + (a - 1)] = adc::mlp_bid(ea, p.clip_hi);
        out[a] = adc::mlp_logp_term(z, ls);
    }
    __syncthreads();
    if (tid < kWave) {       // the first eight lanes: the chains of the log-probability's sum8
        const int c = tid & 7;
        float s = 0.0f;
        if (tid < adc::kMlpChains)
            for (int a = c; a < A; a += adc::kMlpChains) s = s + out[a];
        s = s + __shfl_xor(s, 1, 64);
        s = s + __shfl_xor(s, 2, 64);
        s = s + __shfl_xor(s, 4, 64);
        if (tid == 0) {
            const float lp = kBounded ? 0.0f : adc::mlp_logp_finish(s, A);
            p.logp[env] = lp;
            p.value[env] = s_value;
            if (rec.logp) { rec.logp[env] = lp; rec.value[env] = s_value; }
            p.tick[env] = tick + 1u;          // (every act moves the agent's stream on, as the other agents' acts do)
        }
    }
}

// the env step's side of a recorded day: reward (float32 of the step's float64 reward), terminated, truncated
__global__ void k_mlp_record_outcome(View v, float *__restrict__ reward, uint8_t *__restrict__ term, uint8_t *__restrict__ trunc)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= v.N) return;
    reward[env] = (float)v.reward[env];
    term[env] = v.term[env];
    trunc[env] = v.trunc[env];
}

// an explicit reset forgets the history of the envs it resets (mask null: all)
__global__ void k_mlp_hist_forget(int N, const uint8_t *__restrict__ mask, int32_t *__restrict__ last)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N || (mask && !mask[env])) return;
    last[env] = adc::kMlpHistNone;
}

__global__ void k_mlp_init(MlpView p, int N, const uint64_t *seeds, uint64_t seed, int64_t env_id_base)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N) return;
    p.key[env] = seeds ? adc::mlp_agent_key(seeds[env]) : adc::mlp_default_agent_key(seed, (uint64_t)(env_id_base + env));
    p.tick[env] = 0u;
}
