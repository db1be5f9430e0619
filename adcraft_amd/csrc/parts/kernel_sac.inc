// kernel_sac.inc - soft actor-critic on the device: the soft target under the live actor, the twin critics' pass on the squashed
// action, the actor's reparameterised step through the smaller critic, and the temperature's step.  The arithmetic is
// adc_sac.h's law, the code the host twins adc_sac_target_host / adc_sac_critic_grad_host / adc_sac_actor_grad_host /
// adc_sac_alpha_step_host run.  The ring and its store, the batch indices, the weight gradient, the optimiser step and Polyak
// are kernel_td3.inc's and kernel_pg.inc's, unchanged.  The target is written once, as sac_target_body: k_sac_target here and the
// populations' k_sac_pop_target (kernel_sac_pop.inc) are wrappers that say where a learner's networks, law, key, ring and
// temperature come from.  The critic and the actor kernel and their population twins are each written out (k_sac_critic_sample and
// k_sac_actor_sample say why).
// (part of the single translation unit adc_engine.hip)
// -------------------------------------------------------------------------------------------------
// Shape.  The batch kernels are k_td3_*'s shape: one workgroup of 256 lanes per batch element, the element's row [x | t] and
// every layer's activations in LDS, eight adjacent lanes per neuron with the butterfly join.  The head's per-component values
// (z, sd, w, the two sums' terms, the critic's input gradient) sit behind the delta buffers.  The temperature lives in a device
// cell {log_alpha, m, v, alpha} that k_sac_alpha rewrites at the end of an update and the next update's kernels read through a
// pointer: an update needs no host round trip.  All LDS is the dynamic region.  No atomics; all stores are plain vector stores.
struct SacView {
    adc::Td3Shape sh;
    adc::SacLaw law;
    MlpNet pol, q[2], q_t[2];               // chain-major layers: the live actor, the critics, their targets
    const float *cell;                      // {log_alpha, m, v, alpha}
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
    float *xin;                             // [B][D + A] the gathered rows [x | t]
    float *acts, *deltas, *pieces;          // scratch [B][na], [B][nd], [B][kTd3Pieces]
    int na, nd, maxw;
    // the running normalisers (adc_engine_sac_norm_init; adc_sac_norm.h).  n_shift non-null: the ring's x / x' are raw and are
    // normalised as they are gathered, with the vectors at n_shift / n_scale + member * n_stride.  r_scale non-null: the target is
    // sac_y_norm under the multiplier r_scale[member * r_stride] and r_clip.  Both null: the host launches the batch kernels'
    // NORM = false instantiations, which do not read these fields: their loads and bits are what they were
    // (the fields stand behind the others, whose places in the kernel arguments are what they were)
    const float *n_shift, *n_scale;         // [D] or [M][D]
    size_t n_stride;                        // floats between two members' vectors; 0: shared
    const float *r_scale;                   // [1] or [M]
    int r_stride;                           // 1: a multiplier per member; 0: shared
    float r_clip;
};
enum { kSacCellLogAlpha = 0, kSacCellM = 1, kSacCellV = 2, kSacCellAlpha = 3 };

// floats of LDS: row | the actor's outputs | both critics' outputs | two delta buffers and a dump row | six head vectors | words
__host__ __device__ inline size_t sac_lds_floats(const adc::Td3Shape &sh)
{
    return (size_t)(sh.D + sh.A) + (size_t)adc::td3_outs(sh.pol) + 2u * (size_t)adc::td3_outs(sh.q) + 3u * (size_t)adc::td3_max_width(sh) + 6u * (size_t)sh.A + 8u;
}

struct SacLds {
    float *row, *yp, *yq, *d0, *d1, *dump, *z, *sd, *w, *term, *c, *gq, *words;
};
__device__ __forceinline__ SacLds sac_carve(float *lds, const adc::Td3Shape &sh, int maxw)
{
    SacLds s;
    const int A = sh.A;
    s.row = lds; s.yp = s.row + sh.D + A; s.yq = s.yp + adc::td3_outs(sh.pol); s.d0 = s.yq + 2 * adc::td3_outs(sh.q);
    s.d1 = s.d0 + maxw; s.dump = s.d1 + maxw; s.z = s.dump + maxw; s.sd = s.z + A; s.w = s.sd + A; s.term = s.w + A; s.c = s.term + A;
    s.gq = s.c + A; s.words = s.gq + A;
    return s;
}

// the actor's head on its outputs o[2A] with the stage's draws: t into the row's action part, the per-component values into LDS
__device__ __forceinline__ void sac_heads(int A, int D, uint32_t update, uint64_t key, const adc::SacLaw &law, const SacLds &s, const float *o,
                                          uint32_t stage, uint32_t b)
{
    for (int a = threadIdx.x; a < A; a += kPgBlock) {
        const float z = adc::sac_noise(key, stage, a, b, update);
        const adc::SacHead h = adc::sac_head(o[a], o[A + a], z, law);
        s.row[D + a] = h.t;
        s.z[a] = z; s.sd[a] = h.sd; s.w[a] = h.w; s.term[a] = h.term; s.c[a] = h.c;
    }
    __syncthreads();
}
// lp from the terms in LDS, by the first wave; valid in lane 0 of the first wave, which leaves it in *out
__device__ __forceinline__ void sac_lp(const SacLds &s, int A, float *out)
{
    const int tid = threadIdx.x;
    if (tid < kWave) {
        const int c = tid & 7;
        float st = 0.0f, sc = 0.0f;
        if (tid < adc::kMlpChains)
            for (int a = c; a < A; a += adc::kMlpChains) { st = st + s.term[a]; sc = sc + s.c[a]; }
        st = st + __shfl_xor(st, 1, 64); sc = sc + __shfl_xor(sc, 1, 64);
        st = st + __shfl_xor(st, 2, 64); sc = sc + __shfl_xor(sc, 2, 64);
        st = st + __shfl_xor(st, 4, 64); sc = sc + __shfl_xor(sc, 4, 64);      // adc::mlp_join8, twice
        if (tid == 0) *out = adc::sac_lp_finish(st, sc, A);
    }
    __syncthreads();
}

// The target's body: batch element blockIdx.x of one learner, as in kernel_td3.inc.  p carries what a population's members share;
// what is a learner's own - its networks, law, key, ring and temperature cell - comes as arguments, and `member` moves the
// element's scratch row to member * gridDim.x + blockIdx.x, the normaliser's vectors to member * p.n_stride and its multiplier to
// member * p.r_stride.  The solo kernel passes its view's fields and the literal member 0, which folds those three away.  Without
// a normaliser the host launches the NORM = false instantiations, which do not read the normaliser's fields.

// y of the element
template <bool NORM>
__device__ __forceinline__ void sac_target_body(const SacView &p, const MlpNet &pol, const MlpNet *q_t, const adc::SacLaw &law, uint64_t key,
                                                const Td3Ring &ring, const float *cell, uint32_t member)
{
    extern __shared__ __align__(16) float sac_lds[];
    const adc::Td3Shape &sh = p.sh;
    const int tid = threadIdx.x, D = sh.D;
    const uint32_t b = blockIdx.x;
    const size_t at = (size_t)member * gridDim.x + b;           // the element's scratch row
    const SacLds s = sac_carve(sac_lds, sh, p.maxw);
    const size_t slot = p.p_slot ? (size_t)p.p_slot[at] : (size_t)adc::td3_batch_index(key, b, p.update, p.size);
    const float alpha = cell[kSacCellAlpha];
    const size_t nv = NORM ? (size_t)member * p.n_stride : 0;   // (the member's row of the normaliser's vectors; 0 whenever they are shared)
    // (the multiplier is read here, ahead of the networks' dependent rounds, not behind them where y is formed)
    const float r_mult = NORM && p.r_scale ? p.r_scale[(size_t)member * (size_t)p.r_stride] : 1.0f;
    // (n-step returns: the slot's bootstrap discount in gamma's place, read here for the same reason)
    const float g = ring.gn ? ring.gn[slot] : law.gamma;
    for (int j = tid; j < D; j += kPgBlock) {
        float xj = ring.x2[slot * (size_t)D + j];
        if (NORM && p.n_shift) xj = adc::mlp_normalize(xj, p.n_shift[nv + j], p.n_scale[nv + j]);
        s.row[j] = xj;
    }
    __syncthreads();
    td3_forward(pol, sh.activation, s.row, s.yp, nullptr);
    sac_heads(sh.A, D, p.update, key, law, s, s.yp + adc::td3_hidden(sh.pol), adc::ST_SAC_NEXT, b);
    sac_lp(s, sh.A, s.words + 2);
    const int qlast = adc::td3_hidden(sh.q);
    for (int i = 0; i < 2; ++i) {
        td3_forward(q_t[i], sh.activation, s.row, s.yq, nullptr);
        if (tid == 0) s.words[i] = s.yq[qlast];
        __syncthreads();
    }
    if (tid == 0) {
        const float q = adc::td3_min(s.words[0], s.words[1]);
        p.ybuf[at] = NORM && p.r_scale ? adc::sac_y_norm_g(ring.r[slot], ring.done[slot], q, alpha, s.words[2], g, law, r_mult, p.r_clip)
                                       : adc::sac_y_g(ring.r[slot], ring.done[slot], q, alpha, s.words[2], g, law);
    }
}
template <bool NORM>
__global__ __launch_bounds__(kPgBlock) void k_sac_target(SacView p)
{
    sac_target_body<NORM>(p, p.pol, p.q_t, p.law, p.key, p.ring, p.cell, 0u);
}

// forward and backward of both critics on batch element blockIdx.x: k_td3_critic_sample with t = tanh(ring.a) as the action input.
// This kernel and k_sac_pop_critic_sample stay restated for k_td3_critic_sample's reason: under one sac_critic_body only scalar
// opcodes moved (the same ones), and this kernel ran 105.8 -> 107.0 us (critics 256,256, batch 256, 1024 x 25; two kernel traces a
// side, 390 launches each).  (One pass for both families would be a template over the view type, the NORM switch and the
// transform, handed five carved LDS pointers: more to read than the lines it saves)
template <bool NORM>
__global__ __launch_bounds__(kPgBlock) void k_sac_critic_sample(SacView p)
{
    extern __shared__ __align__(16) float sac_lds[];
    const adc::Td3Shape &sh = p.sh;
    const int tid = threadIdx.x, A = sh.A, D = sh.D, DA = D + A;
    const uint32_t b = blockIdx.x;
    const SacLds s = sac_carve(sac_lds, sh, p.maxw);
    const size_t slot = p.p_slot ? (size_t)p.p_slot[b] : (size_t)adc::td3_batch_index(p.key, b, p.update, p.size);
    float *xin = p.xin + (size_t)b * (size_t)DA;
    for (int j = tid; j < DA; j += kPgBlock) {
        float xj = j < D ? p.ring.x[slot * (size_t)D + j] : adc::mlp_tanh(p.ring.a[slot * (size_t)A + (j - D)]);
        if (NORM && p.n_shift && j < D) xj = adc::mlp_normalize(xj, p.n_shift[j], p.n_scale[j]);
        s.row[j] = xj;
        xin[j] = xj;
    }
    __syncthreads();
    const int nh = adc::td3_hidden(sh.q), no = adc::td3_outs(sh.q);
    float *acts = p.acts + (size_t)b * (size_t)p.na, *deltas = p.deltas + (size_t)b * (size_t)p.nd, *pc = p.pieces + (size_t)b * adc::kTd3Pieces;
    for (int i = 0; i < 2; ++i) {
        td3_forward(p.q[i], sh.activation, s.row, s.yq, acts + i * nh);
        if (tid == 0) {
            const float y = p.ybuf[b], q = s.yq[nh];
            float loss;
            float d = adc::td3_critic_delta(q, y, loss);
            if (p.p_slot) { p.p_absd[2 * (size_t)b + i] = __builtin_fabsf(d); d = p.p_w[b] * d; loss = p.p_w[b] * loss; }
            pc[adc::kTd3Loss1 + i] = loss; pc[adc::kTd3Q1 + i] = q;
            if (i == 0) { pc[adc::kTd3Y] = y; pc[adc::kSacPiLoss] = 0.0f; pc[adc::kSacLp] = 0.0f; pc[adc::kSacPick] = 0.0f; }
            s.d0[0] = d;
            deltas[i * no + nh] = d;
        }
        __syncthreads();
        td3_backward(p.q[i], sh.activation, s.yq, s.d0, s.d1, deltas + i * no, s.dump);
    }
}

// the actor's forward and head, both critics on [x | t], the smaller one's backward through to the action inputs, the head's
// deltas for its 2A outputs, the actor's backward.  This kernel and k_sac_pop_actor_sample stay restated: with one sac_actor_body
// under both, called here with the view's fields and member 0, the compiler no longer reads the picked critic's layers from the
// kernel arguments at pick's offset but selects between the two critics' values, and this kernel's vector opcodes change (NORM
// false: v_cndmask_b32 27 -> 26, v_readfirstlane_b32 2 -> 1, v_cmp_gt_i32 3 -> 4; true: v_cndmask_b32 28 -> 27, v_readfirstlane_b32
// 6 -> 5; registers, scratch and LDS as they were; the twin's vector opcodes did not change), whether the critics came as a
// pointer, as an array reference or under __restrict__
template <bool NORM>
__global__ __launch_bounds__(kPgBlock) void k_sac_actor_sample(SacView p)
{
    extern __shared__ __align__(16) float sac_lds[];
    const adc::Td3Shape &sh = p.sh;
    const int tid = threadIdx.x, A = sh.A, D = sh.D;
    const uint32_t b = blockIdx.x;
    const SacLds s = sac_carve(sac_lds, sh, p.maxw);
    const size_t slot = p.p_slot ? (size_t)p.p_slot[b] : (size_t)adc::td3_batch_index(p.key, b, p.update, p.size);
    const float alpha = p.cell[kSacCellAlpha];
    for (int j = tid; j < D; j += kPgBlock) {
        float xj = p.ring.x[slot * (size_t)D + j];
        if (NORM && p.n_shift) xj = adc::mlp_normalize(xj, p.n_shift[j], p.n_scale[j]);
        s.row[j] = xj;
    }
    __syncthreads();
    float *acts = p.acts + (size_t)b * (size_t)p.na, *deltas = p.deltas + (size_t)b * (size_t)p.nd;
    td3_forward(p.pol, sh.activation, s.row, s.yp, acts);
    const int ph = adc::td3_hidden(sh.pol), qh = adc::td3_hidden(sh.q), no = adc::td3_outs(sh.q);
    const float *o = s.yp + ph;
    sac_heads(A, D, p.update, p.key, p.law, s, o, adc::ST_SAC_PI, b);
    sac_lp(s, A, s.words + 2);
    td3_forward(p.q[0], sh.activation, s.row, s.yq, nullptr);
    td3_forward(p.q[1], sh.activation, s.row, s.yq + no, nullptr);
    // the choice is the same in every lane: both values are read from LDS behind the layers' barrier
    const int pick = __builtin_amdgcn_readfirstlane(adc::sac_pick(s.yq[qh], s.yq[no + qh]));
    const float *yk = s.yq + pick * no;
    if (tid == 0) {
        float *pc = p.pieces + (size_t)b * adc::kTd3Pieces;
        pc[adc::kSacPiLoss] = adc::sac_pi_loss(alpha, s.words[2], yk[qh]);
        pc[adc::kSacLp] = s.words[2];
        pc[adc::kSacPick] = (float)pick;
        s.d0[0] = 1.0f;
    }
    __syncthreads();
    // (pick is a scalar: the picked critic's layers are read from the kernel arguments at a uniform offset)
    const MlpNet &qn = p.q[pick];
    float *dq = td3_backward(qn, sh.activation, yk, s.d0, s.d1, nullptr, s.dump);
    float *dm = dq == s.d0 ? s.d1 : s.d0;
    // (td3_input_back leaves the negated input gradient: gq is its negation, exact)
    td3_input_back(qn.W[0], D, A, sh.q.n_out[0], dq, dm, nullptr, 0, s.gq);
    for (int a = tid; a < A; a += kPgBlock) {
        const float gq = -s.gq[a];
        const float du = adc::sac_du(s.row[D + a], s.w[a], gq, alpha, p.law.eps_sq);
        const float dls = adc::sac_dls(du, s.sd[a], s.z[a], alpha, adc::pg_clamp_moved(o[A + a], 1, p.law.ls_lo, p.law.ls_hi));
        dm[a] = du; dm[A + a] = dls;
        deltas[ph + a] = du; deltas[ph + A + a] = dls;
    }
    __syncthreads();
    td3_backward(p.pol, sh.activation, s.yp, dm, dq, deltas, s.dump);
}

// one step on log_alpha from the joined sum of the actor step's lp; the cell follows.  One wave, lane 0 works
__global__ void k_sac_alpha(float *__restrict__ cell, const double *__restrict__ lp_sum, long long B, float target_entropy, adc::EsStep step)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float m = cell[kSacCellM], v = cell[kSacCellV], alpha;
    const float la = adc::sac_alpha_step(step, cell[kSacCellLogAlpha], adc::sac_alpha_grad(lp_sum[0], B, target_entropy), m, v, alpha);
    cell[kSacCellLogAlpha] = la; cell[kSacCellM] = m; cell[kSacCellV] = v; cell[kSacCellAlpha] = alpha;
}
