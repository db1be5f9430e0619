// kernel_td3.inc - off-policy training on the device: the replay ring filled from the rollout record, the TD3 target, the twin
// critics' forward and backward pass, the deterministic policy gradient through critic 1's input, and Polyak averaging.  The
// arithmetic is adc_td3.h's law, the code the host twins adc_td3_target_host / adc_td3_critic_grad_host /
// adc_td3_actor_grad_host run.  The store, the target, the actor's pass and Polyak are each written once, as a td3_*_body
// function: the solo kernels k_td3_* here and the populations' k_td3_pop_* (kernel_td3_pop.inc) are wrappers that say where a
// learner's networks, law, key and ring come from - the view's fields and member 0 here, row blockIdx.y of the members' tables
// there.  The critic kernel and its twin are each written out (k_td3_critic_sample says why).
// (part of the single translation unit adc_engine.hip)
// -------------------------------------------------------------------------------------------------
// Shape.  The batch kernels are k_pg_sample's shape: one workgroup of 256 lanes per batch element, the element's input row
// [x | an] and every layer's activations in LDS, eight adjacent lanes per neuron with the butterfly join (mlp_layer one way,
// pg_layer_back the other).  Every workgroup derives its ring slot from the batch's counter-addressed draw, so no index
// buffer is written first.  The critic kernel leaves the gathered rows, the hidden activations and the deltas in scratch; the
// weight gradient over the batch is k_pg_wgrad / k_pg_grad_join unchanged (X = the gathered rows for a first layer), the
// optimiser step k_pg_update on a PgLayout over the critics' (or the policy's) chain-major stores.  All LDS is the dynamic
// region (no static words in front of it).  No atomics; all stores are plain vector stores.
struct Td3Ring {
    float *x, *a, *r, *x2;                  // [C][D], [C][A], [C], [C][D]
    uint8_t *done;                          // [C]
    float *gn;                              // [C] the slot's bootstrap discount (adc_engine_replay_nstep_init; adc_td3.h "n-step"), or null
};

struct Td3View {
    adc::Td3Shape sh;
    adc::Td3Law law;
    MlpNet pol, pol_t, q[2], q_t[2];        // chain-major layers: the live actor, its target, the critics, their targets
    const float *a_shift, *a_scale;         // [A] (sh.norm)
    // the running normalisers (adc_engine_td3_norm_init; adc_td3_norm.h).  n_shift non-null: the ring's x / x' are raw and are
    // normalised as they are gathered, with the vectors at n_shift / n_scale + member * n_stride.  r_scale non-null: the target is
    // td3_y_norm under the multiplier r_scale[member * r_stride] and r_clip.  Both null: the kernels' loads and bits are what they were
    const float *n_shift, *n_scale;         // [D] or [M][D]
    size_t n_stride;                        // floats between two members' vectors; 0: shared
    const float *r_scale;                   // [1] or [M]
    int r_stride;                           // 1: a multiplier per member; 0: shared
    float r_clip;
    // prioritised replay (adc_engine_replay_prio_init; adc_per.h, parts/kernel_per.inc).  p_slot non-null: the element's ring slot is
    // p_slot[element] in place of td3_batch_index, the critics' output deltas and loss pieces are weighted by p_w[element], and the
    // critic kernel leaves |d_1|, |d_2| at p_absd[2 element].  Null: the kernels' loads and bits are what they were
    const int32_t *p_slot;                  // [B] or [M][B]
    const float *p_w;
    float *p_absd;
    Td3Ring ring;
    uint32_t size, update;                  // the ring's size; the update's number
    uint64_t key;
    float *ybuf;                            // [B]
    float *xin;                             // [B][D + A] the gathered rows
    float *acts, *deltas, *pieces;          // scratch [B][na], [B][nd], [B][kTd3Pieces]
    int na, nd, maxw;
};

// floats of LDS: row | the actor's outputs | one critic's outputs | two delta buffers | a dump row
__host__ __device__ inline size_t td3_lds_floats(const adc::Td3Shape &sh)
{
    return (size_t)(sh.D + sh.A) + (size_t)adc::td3_outs(sh.pol) + (size_t)adc::td3_outs(sh.q) + 3u * (size_t)adc::td3_max_width(sh) + 4u;
}

// a network forward on the LDS row `in`, every layer's outputs kept at ys (layers in order); the hidden ones written to g_acts
__device__ __forceinline__ void td3_forward(const MlpNet &net, int activation, const float *in, float *ys, float *__restrict__ g_acts)
{
    const int tid = threadIdx.x;
    float *y = ys;
    int ao = 0;
    for (int l = 0; l < net.layers; ++l) {
        const bool last = l + 1 == net.layers;
        const int n_out = net.n_out[l];
        mlp_layer(net.W[l], net.b[l], net.n_in[l], n_out, in, y, last ? -1 : activation);
        if (!last && g_acts) {
            for (int h = tid; h < n_out; h += kPgBlock) g_acts[ao + h] = y[h];
            ao += n_out;
        }
        in = y; y += n_out;
    }
}

// the hidden deltas of a network whose last layer's deltas are in dcur, last to first; g_deltas: the sample's deltas of this
// network (layers in order), or null: only LDS (dump receives what pg_layer_back writes out).  Returns where layer 0's deltas are.
__device__ __forceinline__ float *td3_backward(const MlpNet &net, int activation, const float *ys, float *dcur, float *dnew, float *g_deltas,
                                               float *dump)
{
    int off[adc::kMlpMaxLayers], o = 0;
    for (int l = 0; l < net.layers; ++l) { off[l] = o; o += net.n_out[l]; }
    for (int l = net.layers - 2; l >= 0; --l) {
        pg_layer_back(net.W[l + 1], net.n_out[l], net.n_out[l + 1], ys + off[l], dcur, dnew, activation, g_deltas ? g_deltas + off[l] : dump);
        float *t = dcur; dcur = dnew; dnew = t;
    }
    return dcur;
}

// dmu[a] = -(din[D + a] * a_scale[a]): the first critic layer's deltas carried to the action inputs, no activation derivative
// kBounded: dmu[a] = -(din[D + a] * (1 - t[a]^2)) through the bounded actor's tanh, `scale` naming the row's t = tanh(mu) (adc_td3.h
// "bounded"); without it the code is what it was
template <bool kBounded = false>
__device__ __forceinline__ void td3_input_back(const float *__restrict__ W, int j0, int n, int n_out, const float *dcur, float *dnew,
                                               const float *__restrict__ scale, int norm, float *__restrict__ g_out)
{
    const int tid = threadIdx.x;
    const int pairs = n * adc::kMlpChains;
    for (int p0 = 0; p0 < pairs; p0 += kPgBlock) {
        const int pi = p0 + tid;
        const bool on = pi < pairs;
        const int a = on ? pi >> 3 : 0, c = pi & 7;
        float acc = 0.0f;
        if (on)
            for (int h = c; h < n_out; h += adc::kMlpChains) acc = adc::mlp_mac(acc, W[adc::mlp_weight_index(j0 + a, h, n_out)], dcur[h]);
        float s = acc;
        s = s + __shfl_xor(s, 1, 64);
        s = s + __shfl_xor(s, 2, 64);
        s = s + __shfl_xor(s, 4, 64);           // adc::mlp_join8
        if (on && c == 0) {
            float d;
            if constexpr (kBounded) d = adc::td3_dmu_bounded(s, scale[a]);
            else d = adc::td3_dmu(s, norm ? scale[a] : 0.0f, norm);
            dnew[a] = d;
            g_out[a] = d;
        }
    }
    __syncthreads();
}

// sample s = (t - t0) * n + local env of the recorded days [t0, t1) of the member's envs [member n, (member + 1) n) into slot
// (written + s) mod C of its ring
// kHist: the policy has an observation history (adc_mlp.h): the last day's x' is the stacked row, peeked (nothing is written)
// kNstep: n-step returns (adc_td3.h "n-step"): r, done and gn are the window's of `nstep` days under `gamma`, x' the row m days on.
// Every lane walks the window (at most nstep dependent loads at workgroup-uniform addresses); without it the code is what it was
template <bool kHist = false, bool kNstep = false>
__device__ __forceinline__ void td3_store_body(const View &v, const float *__restrict__ shift, const float *__restrict__ scale, int D, int A,
                                               const float *__restrict__ ro_obs, const float *__restrict__ ro_action,
                                               const float *__restrict__ ro_reward, const uint8_t *__restrict__ ro_term,
                                               const uint8_t *__restrict__ ro_trunc, int t0, int t1, int n, int member, const Td3Ring ring,
                                               unsigned long long written, unsigned long long C, const float *__restrict__ hist = nullptr,
                                               const int32_t *__restrict__ h_last = nullptr, const int32_t *__restrict__ h_from = nullptr,
                                               int frames = 1, int nstep = 1, float gamma = 0.0f)
{
    const int tid = threadIdx.x, N = v.N;
    const unsigned long long s = blockIdx.x, count = (unsigned long long)(t1 - t0) * (unsigned long long)n;
    if (s >= count || s + C < count) return;            // (a later sample of this store lands on the same slot)
    const int t = t0 + (int)(s / (unsigned long long)n), env = member * n + (int)(s % (unsigned long long)n);
    const size_t slot = (size_t)((written + s) % C), row = (size_t)t * (size_t)N + (size_t)env;
    for (int j = tid; j < D; j += kPgBlock) ring.x[slot * (size_t)D + j] = ro_obs[row * (size_t)D + j];
    for (int a = tid; a < A; a += kPgBlock) ring.a[slot * (size_t)A + a] = ro_action[row * (size_t)A + a];
    int m = 1;
    if constexpr (kNstep) {
        const adc::Td3Window w = adc::td3_nstep_window(ro_reward + row, ro_term + row, ro_trunc + row, (size_t)N, t1 - t, nstep, gamma);
        m = w.m;
        if (tid == 0) {
            ring.r[slot] = w.R;
            ring.done[slot] = (uint8_t)w.done;
            ring.gn[slot] = w.g;
        }
    } else if (tid == 0) {
        ring.r[slot] = ro_reward[row];
        ring.done[slot] = (uint8_t)((ro_term[row] | ro_trunc[row]) ? 1 : 0);
    }
    if (t + m < t1) {
        const size_t next = row + (size_t)m * (size_t)N;
        for (int j = tid; j < D; j += kPgBlock) ring.x2[slot * (size_t)D + j] = ro_obs[next * (size_t)D + j];
    } else {
        // the input row an act would read now (k_mlp_policy's prologue)
        const int32_t d = v.day[env];
        const bool first = d == 0;
        const double cum = v.cum_profit[env];
        const int32_t days = v.day_out[env];
        int32_t from = 0;
        if constexpr (kHist) from = adc::mlp_hist_from(d, h_last[env], h_from[env]);
        for (int j = tid; j < D; j += kPgBlock) {
            float xj = mlp_row_raw_at<kHist>(v, hist, frames, env, j, first, cum, days, d, from);
            if (shift) xj = adc::mlp_normalize(xj, shift[j], scale[j]);
            ring.x2[slot * (size_t)D + j] = xj;
        }
    }
}
__global__ __launch_bounds__(kPgBlock) void k_td3_store(View v, const float *__restrict__ shift, const float *__restrict__ scale, int D, int A,
                                                        const float *__restrict__ ro_obs, const float *__restrict__ ro_action,
                                                        const float *__restrict__ ro_reward, const uint8_t *__restrict__ ro_term,
                                                        const uint8_t *__restrict__ ro_trunc, int t0, int t1, Td3Ring ring,
                                                        unsigned long long written, unsigned long long C)
{
    td3_store_body(v, shift, scale, D, A, ro_obs, ro_action, ro_reward, ro_term, ro_trunc, t0, t1, v.N, 0, ring, written, C);
}
// ... with an observation history (adc_engine_mlp_init_frames, frames > 1)
__global__ __launch_bounds__(kPgBlock) void k_td3_store_hist(View v, const float *__restrict__ shift, const float *__restrict__ scale, int D, int A,
                                                             const float *__restrict__ ro_obs, const float *__restrict__ ro_action,
                                                             const float *__restrict__ ro_reward, const uint8_t *__restrict__ ro_term,
                                                             const uint8_t *__restrict__ ro_trunc, int t0, int t1, Td3Ring ring,
                                                             unsigned long long written, unsigned long long C, const float *__restrict__ hist,
                                                             const int32_t *__restrict__ h_last, const int32_t *__restrict__ h_from, int frames)
{
    td3_store_body<true>(v, shift, scale, D, A, ro_obs, ro_action, ro_reward, ro_term, ro_trunc, t0, t1, v.N, 0, ring, written, C, hist, h_last,
                         h_from, frames);
}

// ... with n-step returns (adc_engine_replay_nstep_init): the learner's gamma comes with the launch
__global__ __launch_bounds__(kPgBlock) void k_td3_store_nstep(View v, const float *__restrict__ shift, const float *__restrict__ scale, int D, int A,
                                                              const float *__restrict__ ro_obs, const float *__restrict__ ro_action,
                                                              const float *__restrict__ ro_reward, const uint8_t *__restrict__ ro_term,
                                                              const uint8_t *__restrict__ ro_trunc, int t0, int t1, Td3Ring ring,
                                                              unsigned long long written, unsigned long long C, int nstep, float gamma)
{
    td3_store_body<false, true>(v, shift, scale, D, A, ro_obs, ro_action, ro_reward, ro_term, ro_trunc, t0, t1, v.N, 0, ring, written, C, nullptr,
                                nullptr, nullptr, 1, nstep, gamma);
}
__global__ __launch_bounds__(kPgBlock) void k_td3_store_hist_nstep(View v, const float *__restrict__ shift, const float *__restrict__ scale, int D,
                                                                   int A, const float *__restrict__ ro_obs, const float *__restrict__ ro_action,
                                                                   const float *__restrict__ ro_reward, const uint8_t *__restrict__ ro_term,
                                                                   const uint8_t *__restrict__ ro_trunc, int t0, int t1, Td3Ring ring,
                                                                   unsigned long long written, unsigned long long C,
                                                                   const float *__restrict__ hist, const int32_t *__restrict__ h_last,
                                                                   const int32_t *__restrict__ h_from, int frames, int nstep, float gamma)
{
    td3_store_body<true, true>(v, shift, scale, D, A, ro_obs, ro_action, ro_reward, ro_term, ro_trunc, t0, t1, v.N, 0, ring, written, C, hist, h_last,
                               h_from, frames, nstep, gamma);
}

__global__ void k_td3_indices(uint64_t key, uint32_t update, uint32_t size, int B, int32_t *__restrict__ out)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) out[b] = (int32_t)adc::td3_batch_index(key, (uint32_t)b, update, size);
}

// The batch bodies: batch element blockIdx.x of one learner.  p carries what a population's members share (the shapes, the action
// normalisation, the ring's size, the update's number, the scratch, na / nd / maxw); what is a learner's own - its networks, law,
// key and ring - comes as arguments, and `member` moves the element's scratch row to member * gridDim.x + blockIdx.x, the
// normaliser's vectors to member * p.n_stride and its multiplier to member * p.r_stride.  The solo kernels pass their view's
// fields and the literal member 0, which folds those three away.

// y of the element.  kBounded (adc_td3.h "bounded"): the target actor's mean goes through tanh and the target action is clipped to
// [-1, 1]; without it the code is what it was
template <bool kBounded = false>
__device__ __forceinline__ void td3_target_body(const Td3View &p, const MlpNet &pol_t, const MlpNet *q_t, const adc::Td3Law &law, uint64_t key,
                                                const Td3Ring &ring, uint32_t member)
{
    extern __shared__ __align__(16) float td3_lds[];
    const adc::Td3Shape &sh = p.sh;
    const int tid = threadIdx.x, A = sh.A, D = sh.D;
    const uint32_t b = blockIdx.x;
    const size_t at = (size_t)member * gridDim.x + b;           // the element's scratch row
    float *row = td3_lds, *yp = row + D + A, *yq = yp + adc::td3_outs(sh.pol), *words = yq + adc::td3_outs(sh.q) + 3 * p.maxw;
    const size_t slot = p.p_slot ? (size_t)p.p_slot[at] : (size_t)adc::td3_batch_index(key, b, p.update, p.size);
    const size_t nv = (size_t)member * p.n_stride;              // (the member's row of the normaliser's vectors; 0 whenever they are shared)
    // (the multiplier is read here, ahead of the networks' dependent rounds, not behind them where y is formed)
    const float r_mult = p.r_scale ? p.r_scale[(size_t)member * (size_t)p.r_stride] : 1.0f;
    // (n-step returns: the slot's bootstrap discount in gamma's place, read here for the same reason)
    const float g = ring.gn ? ring.gn[slot] : law.gamma;
    for (int j = tid; j < D; j += kPgBlock) {
        float xj = ring.x2[slot * (size_t)D + j];
        if (p.n_shift) xj = adc::mlp_normalize(xj, p.n_shift[nv + j], p.n_scale[nv + j]);
        row[j] = xj;
    }
    __syncthreads();
    td3_forward(pol_t, sh.activation, row, yp, nullptr);
    const float *mu = yp + adc::td3_hidden(sh.pol);
    if constexpr (kBounded) {
        const adc::Td3Law box = adc::td3_law_bounded(law);
        for (int a = tid; a < A; a += kPgBlock) row[D + a] = adc::td3_target_action(adc::mlp_tanh(mu[a]), adc::td3_noise(key, a, b, p.update), box);
    } else {
        for (int a = tid; a < A; a += kPgBlock) {
            const float ap = adc::td3_target_action(mu[a], adc::td3_noise(key, a, b, p.update), law);
            row[D + a] = adc::td3_action_norm(ap, p.a_shift, p.a_scale, a, sh.norm);
        }
    }
    __syncthreads();
    const int qlast = adc::td3_hidden(sh.q);
    for (int i = 0; i < 2; ++i) {
        td3_forward(q_t[i], sh.activation, row, yq, nullptr);
        if (tid == 0) words[i] = yq[qlast];
        __syncthreads();
    }
    if (tid == 0) {
        const float q = adc::td3_min(words[0], words[1]);
        p.ybuf[at] = p.r_scale ? adc::td3_y_norm_g(ring.r[slot], ring.done[slot], q, g, law, r_mult, p.r_clip)
                               : adc::td3_y_g(ring.r[slot], ring.done[slot], q, g, law);
    }
}
__global__ __launch_bounds__(kPgBlock) void k_td3_target(Td3View p)
{
    td3_target_body(p, p.pol_t, p.q_t, p.law, p.key, p.ring, 0u);
}
__global__ __launch_bounds__(kPgBlock) void k_td3_target_bounded(Td3View p)
{
    td3_target_body<true>(p, p.pol_t, p.q_t, p.law, p.key, p.ring, 0u);
}

// forward and backward of both critics on batch element blockIdx.x.  This kernel and k_td3_pop_critic_sample stay restated: under
// one td3_critic_body, called here with the view's fields and member 0, registers, scratch, LDS and every vector, LDS and memory
// opcode count of both kernels were the restated form's and only scalar opcodes moved (here s_add_i32 66 -> 63, s_mul_i32 27 -> 24,
// s_cbranch_vccnz 16 -> 15, s_cbranch_vccz 5 -> 6, s_and_b64 16 -> 15, s_andn2_b64 16 -> 17), but this kernel ran 115.3 -> 119.6 us
// (critics 256,256, batch 256, 1024 x 25; two kernel traces a side, 396 launches each) and TD3's per update of 64 went 0.3304 ->
// 0.3337 ms, outside the restated form's own spread (profiles/pr_offpolicy_kernel_bodies.txt)
__global__ __launch_bounds__(kPgBlock) void k_td3_critic_sample(Td3View p)
{
    extern __shared__ __align__(16) float td3_lds[];
    const adc::Td3Shape &sh = p.sh;
    const int tid = threadIdx.x, A = sh.A, D = sh.D, DA = D + A;
    const uint32_t b = blockIdx.x;
    float *row = td3_lds, *yq = row + DA + adc::td3_outs(sh.pol), *d0 = yq + adc::td3_outs(sh.q), *d1 = d0 + p.maxw, *dump = d1 + p.maxw;
    const size_t slot = p.p_slot ? (size_t)p.p_slot[b] : (size_t)adc::td3_batch_index(p.key, b, p.update, p.size);
    float *xin = p.xin + (size_t)b * (size_t)DA;
    for (int j = tid; j < DA; j += kPgBlock) {
        float xj = j < D ? p.ring.x[slot * (size_t)D + j]
                         : adc::td3_action_norm(p.ring.a[slot * (size_t)A + (j - D)], p.a_shift, p.a_scale, j - D, sh.norm);
        if (p.n_shift && j < D) xj = adc::mlp_normalize(xj, p.n_shift[j], p.n_scale[j]);
        row[j] = xj;
        xin[j] = xj;
    }
    __syncthreads();
    const int nh = adc::td3_hidden(sh.q), no = adc::td3_outs(sh.q);
    float *acts = p.acts + (size_t)b * (size_t)p.na, *deltas = p.deltas + (size_t)b * (size_t)p.nd, *pc = p.pieces + (size_t)b * adc::kTd3Pieces;
    for (int i = 0; i < 2; ++i) {
        td3_forward(p.q[i], sh.activation, row, yq, acts + i * nh);
        if (tid == 0) {
            const float y = p.ybuf[b], q = yq[nh];
            float loss;
            float d = adc::td3_critic_delta(q, y, loss);
            if (p.p_slot) { p.p_absd[2 * (size_t)b + i] = __builtin_fabsf(d); d = p.p_w[b] * d; loss = p.p_w[b] * loss; }
            pc[adc::kTd3Loss1 + i] = loss; pc[adc::kTd3Q1 + i] = q;
            if (i == 0) { pc[adc::kTd3Y] = y; pc[adc::kTd3QPi] = 0.0f; pc[6] = 0.0f; pc[7] = 0.0f; }
            d0[0] = d;
            deltas[i * no + nh] = d;
        }
        __syncthreads();
        td3_backward(p.q[i], sh.activation, yq, d0, d1, deltas + i * no, dump);
    }
}

// the actor's forward, critic 1 on [x | norm(mu)], its backward through to the action inputs, the actor's backward
// kBounded (adc_td3.h "bounded"): critic 1 on [x | tanh(mu)], and the tanh's derivative on the way back; without it the code is what it was
template <bool kBounded = false>
__device__ __forceinline__ void td3_actor_body(const Td3View &p, const MlpNet &pol, const MlpNet &q1, uint64_t key, const Td3Ring &ring,
                                               uint32_t member)
{
    extern __shared__ __align__(16) float td3_lds[];
    const adc::Td3Shape &sh = p.sh;
    const int tid = threadIdx.x, A = sh.A, D = sh.D;
    const uint32_t b = blockIdx.x;
    const size_t at = (size_t)member * gridDim.x + b;
    float *row = td3_lds, *yp = row + D + A, *yq = yp + adc::td3_outs(sh.pol), *d0 = yq + adc::td3_outs(sh.q), *d1 = d0 + p.maxw, *dump = d1 + p.maxw;
    const size_t slot = p.p_slot ? (size_t)p.p_slot[at] : (size_t)adc::td3_batch_index(key, b, p.update, p.size);
    const size_t nv = (size_t)member * p.n_stride;
    for (int j = tid; j < D; j += kPgBlock) {
        float xj = ring.x[slot * (size_t)D + j];
        if (p.n_shift) xj = adc::mlp_normalize(xj, p.n_shift[nv + j], p.n_scale[nv + j]);
        row[j] = xj;
    }
    __syncthreads();
    float *acts = p.acts + at * (size_t)p.na, *deltas = p.deltas + at * (size_t)p.nd;
    td3_forward(pol, sh.activation, row, yp, acts);
    const int ph = adc::td3_hidden(sh.pol), qh = adc::td3_hidden(sh.q);
    if constexpr (kBounded) {
        for (int a = tid; a < A; a += kPgBlock) row[D + a] = adc::mlp_tanh(yp[ph + a]);
    } else {
        for (int a = tid; a < A; a += kPgBlock) row[D + a] = adc::td3_action_norm(yp[ph + a], p.a_shift, p.a_scale, a, sh.norm);
    }
    __syncthreads();
    td3_forward(q1, sh.activation, row, yq, nullptr);
    if (tid == 0) {
        p.pieces[at * adc::kTd3Pieces + adc::kTd3QPi] = yq[qh];
        d0[0] = 1.0f;
    }
    __syncthreads();
    float *dq = td3_backward(q1, sh.activation, yq, d0, d1, nullptr, dump);
    float *dm = dq == d0 ? d1 : d0;
    if constexpr (kBounded) td3_input_back<true>(q1.W[0], D, A, sh.q.n_out[0], dq, dm, row + D, 0, deltas + ph);
    else td3_input_back(q1.W[0], D, A, sh.q.n_out[0], dq, dm, p.a_scale, sh.norm, deltas + ph);
    td3_backward(pol, sh.activation, yp, dm, dq, deltas, dump);
}
__global__ __launch_bounds__(kPgBlock) void k_td3_actor_sample(Td3View p)
{
    td3_actor_body(p, p.pol, p.q[0], p.key, p.ring, 0u);
}
__global__ __launch_bounds__(kPgBlock) void k_td3_actor_sample_bounded(Td3View p)
{
    td3_actor_body<true>(p, p.pol, p.q[0], p.key, p.ring, 0u);
}

// target = target + tau * (param - target) on the member's [Q] of the flat vectors, the targets' chain-major stores (L member 0's,
// a member's `stride` floats further each) rebuilt from the result
__device__ __forceinline__ void td3_polyak_body(const PgLayout &L, size_t stride, float *__restrict__ target, const float *__restrict__ param,
                                                float tau, size_t member)
{
    const int p = blockIdx.x * kPgBlock + threadIdx.x;
    if (p >= L.Q) return;
    const size_t i = member * (size_t)L.Q + (size_t)p;
    const float t1 = adc::td3_polyak(target[i], param[i], tau);
    target[i] = t1;
    *(pg_param_slot(L, p) + member * stride) = t1;
}
__global__ __launch_bounds__(kPgBlock) void k_td3_polyak(PgLayout L, float *__restrict__ target, const float *__restrict__ param, float tau)
{
    td3_polyak_body(L, 0, target, param, tau, 0);
}
