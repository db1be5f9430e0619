// kernel_mlp_gru.inc - the recurrent learned agent on the device: the policy of parts/kernel_mlp_policy.inc with one GRU cell in
// front of its output layer, and the per-env state the cell carries from one act to the next.  The arithmetic is adc_gru.h's law
// (and adc_mlp.h's for everything round the cell), the code the host twin adc_mlp_act_recurrent_host runs too.
// (part of the single translation unit adc_engine.hip)
// -------------------------------------------------------------------------------------------------
// Shape.  As the feed-forward act: one workgroup of 256 lanes per env, the input row and the activations in LDS.  The cell's two
// matrix products are two calls of mlp_layer with n_out = 3G - Wi on the trunk's activation, Wh on the old state - into 6G floats
// of LDS; one lane per unit then forms the gates and the new state.  The old state is read from the slot the last act wrote (or
// is zeros) before the first barrier, the new one goes to the other slot after the cell: a second act on the same day finds the
// input state it found the first time.  The act is a kernel of its own, so that every instantiation of k_mlp_policy is the code
// it was; the bootstrap value (mode 1 there) reads no state and stays that kernel's.
struct MlpGruView {
    float *h;                               // [N][2][G] the state, slot = episode day & 1
    int32_t *last, *from;                   // [N] the episode day of the last act (-2: none); the day the state's run began
    int G;                                  // the cell's width; 0: the policy is feed-forward
    int at;                                 // the trunk's layers: MlpView::pol's layers 0 .. at-1; its layer `at` is the output layer [G][P]
    int n_in;                               // the cell's input: the trunk's last width, or D without a trunk
    const float *Wi, *bi, *Wh, *bh;         // the centre's cell: two chain-major layers with n_out = 3G
    // a member's cell and output layer, floats from its base (the trunk's are MlpView::pop_offW / pop_offb: the flat order's first terms)
    uint32_t pop_Wi, pop_bi, pop_Wh, pop_bh, pop_Wo, pop_bo;
};

// floats of LDS of the recurrent act: the feed-forward act's | the state | gi | gh
__host__ __device__ inline size_t mlp_gru_lds_floats(int D, int P, int G) { return mlp_lds_floats(D, P) + adc::gru_lds_floats(G); }

// kMembers 0: every env runs `pol` and the centre's cell;  1: the env's trunk, cell and output layer are its member's (a population)
template <int kMembers>
__global__ __launch_bounds__(kMlpBlock) void k_mlp_policy_gru(View v, MlpView p, MlpGruView g, const float *__restrict__ replay_z, float budget_override,
                                                              float *__restrict__ bids, float *__restrict__ budgets, MlpRecordSlot rec)
{
    extern __shared__ __align__(16) float gru_lds[];
    __shared__ float s_value;
    const int tid = threadIdx.x, K = v.K, D = p.D, A = p.A, G = g.G, env = blockIdx.x;
    float *h0 = gru_lds + D, *h1 = h0 + adc::kMlpMaxWidth;
    float *out = gru_lds + D + 2 * adc::kMlpMaxWidth;
    float *hs = out + p.P, *gi = hs + G, *gh = gi + 3 * G;
    const int32_t d = v.day[env];
    const int32_t from = adc::mlp_hist_from(d, g.last[env], g.from[env]);
    {
        // the input row: zeros on the first day of an episode (the reset observation), else the last step's outputs
        const bool first = d == 0;
        const size_t o = (size_t)env * K;
        const double cum = v.cum_profit[env];
        const int32_t days = v.day_out[env];
        for (int j = tid; j < D; j += kMlpBlock) {
            float xj = first ? 0.0f : adc::mlp_obs_at(j, K, v.clk + o, v.cost + o, v.imp + o, v.rev + o, v.conv + o, cum, days);
            const float raw = xj;
            if (p.shift) xj = adc::mlp_normalize(xj, p.shift[j], p.scale[j]);
            gru_lds[j] = xj;
            if (rec.obs) rec.obs[(size_t)env * D + j] = rec.raw_obs ? raw : xj;
        }
        // the input state: zeros where a run begins, else what the act of the day before (or an earlier act of this day) read too
        const bool zeros = adc::gru_starts_from_zeros(d, from);
        const float *src = g.h + ((size_t)env * 2u + (size_t)adc::gru_read_slot(d)) * (size_t)G;
        for (int j = tid; j < G; j += kMlpBlock) hs[j] = zeros ? 0.0f : src[j];
        __syncthreads();
    }
    if (p.val.layers > 0) {
        // (the value network's single output lands in the first float of `out`, which the policy network overwrites afterwards)
        mlp_network<false>(p.val, p, nullptr, p.activation, gru_lds, D, out);
        if (tid == 0) s_value = out[0];
        __syncthreads();
    } else if (tid == 0) s_value = 0.0f;
    const float *mbase = kMembers == 1 ? p.pop + (size_t)p.member[env] * p.pop_stride : nullptr;
    // the trunk, the activation after each of its layers
    const float *x = gru_lds;
    for (int l = 0; l < g.at; ++l) {
        float *y = (l & 1) ? h1 : h0;
        mlp_layer(kMembers == 1 ? mbase + p.pop_offW[l] : p.pol.W[l], kMembers == 1 ? mbase + p.pop_offb[l] : p.pol.b[l], p.pol.n_in[l], p.pol.n_out[l], x, y,
                  p.activation);
        x = y;
    }
    // the cell: gi = Wi x + bi, gh = Wh h + bh, then one lane per unit
    mlp_layer(kMembers == 1 ? mbase + g.pop_Wi : g.Wi, kMembers == 1 ? mbase + g.pop_bi : g.bi, g.n_in, 3 * G, x, gi, -1);
    mlp_layer(kMembers == 1 ? mbase + g.pop_Wh : g.Wh, kMembers == 1 ? mbase + g.pop_bh : g.bh, G, 3 * G, hs, gh, -1);
    {
        float *dst = g.h + ((size_t)env * 2u + (size_t)adc::gru_write_slot(d)) * (size_t)G;
        for (int j = tid; j < G; j += kMlpBlock) {
            const float hn = adc::gru_unit(gi[j], gh[j], gi[G + j], gh[G + j], gi[2 * G + j], gh[2 * G + j], hs[j]);
            hs[j] = hn;                     // (a lane reads and writes its own units alone)
            dst[j] = hn;
        }
        if (tid == 0) { g.last[env] = d; g.from[env] = from; }
        __syncthreads();
    }
    mlp_layer(kMembers == 1 ? mbase + g.pop_Wo : p.pol.W[g.at], kMembers == 1 ? mbase + g.pop_bo : p.pol.b[g.at], G, p.P, hs, out, -1);
    // heads, sample, the env's action; the log-probability's terms replace the means in LDS (k_mlp_policy's statements)
    const uint64_t key = p.key[env];
    const uint32_t tick = p.tick[env];
    for (int a = tid; a < A; a += kMlpBlock) {
        const float mean = out[a];
        const float ls = adc::mlp_clamp_log_std(p.two_heads ? out[A + a] : p.log_std[a], p.clamp, p.ls_lo, p.ls_hi);
        float z = 0.0f;
        if (!p.deterministic) z = replay_z ? replay_z[(size_t)env * A + a] : adc::mlp_normal(key, tick, a);
        const float act = adc::mlp_sample(mean, ls, z, p.deterministic);
        const size_t oa = (size_t)env * A + a;
        p.mean[oa] = mean;
        p.ls[oa] = ls;
        p.action[oa] = act;
        if (rec.action) rec.action[oa] = act;
        if (a == 0) budgets[env] = adc::mlp_budget(act, budget_override);
        else bids[(size_t)env * K + (a - 1)] = adc::mlp_bid(act, p.clip_hi);
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
            const float lp = adc::mlp_logp_finish(s, A);
            p.logp[env] = lp;
            p.value[env] = s_value;
            if (rec.logp) { rec.logp[env] = lp; rec.value[env] = s_value; }
            p.tick[env] = tick + 1u;
        }
    }
}
