// kernel_sac_pop.inc - SAC learner populations (adc_engine_sac_pop_*): M soft actor-critic learners in lock-step, every launch over
// all members.  The member is one more grid dimension, as in kernel_td3_pop.inc: what is a member's own is read from the device
// tables MlpLearner[M] (its live actor), Td3Member[M] (its td3 key, its critics, target critics and ring; law.tau for Polyak; pol_t
// is not used), SacMember[M] (its law constants, its target entropy, its temperature cell) and Td3PopStep[M] (the next step's clip
// scale and optimiser constants).  The arithmetic is adc_sac.h's law through the helpers kernel_sac.inc and kernel_td3.inc use
// (td3_forward, td3_backward, td3_input_back, sac_heads, sac_lp, adc::sac_*): a member runs the solo code on its own ring under
// its own key, so its bits are a solo engine's, whatever M and the other members are.  The batch kernels restate the solo kernels'
// bodies rather than share them: kernel_sac.inc's bodies stay the solo learner's alone.  The store, the weight gradient,
// its join, the chunked sums, the optimiser step and Polyak are k_td3_pop_store / k_pg_pop_wgrad / k_pg_pop_grad_join /
// k_pg_pop_chunk_sums / k_pg_pop_join / k_td3_pop_step / k_td3_pop_polyak unchanged.  All LDS is the dynamic region; no atomics;
// all stores are plain vector stores.
// (part of the single translation unit adc_engine.hip)
struct SacMember {
    adc::SacLaw law;
    float target_entropy;
    float *cell;                            // the member's {log_alpha, m, v, alpha}: its four floats of the [M][4] array
};

// The batch kernels: batch element blockIdx.x of member blockIdx.y.  p carries what the members share (the shapes, the ring's
// size, the update's number, the scratch for all members, na / nd / maxw); p.law, p.pol, p.q, p.q_t, p.cell, p.ring and p.key are
// not read.  A member's scratch rows, ybuf and pieces start at member * gridDim.x.  Under a running normaliser (p.n_shift / p.r_scale
// non-null; adc_sac_norm.h) the member's vectors are at member * p.n_stride, its multiplier at member * p.r_stride: the NORM = true
// instantiations; without one the host launches NORM = false, which does not read those fields.

// what sac_heads reads of a view - the sizes, the update's number, the key, the law - with the member's key and law.  (The rest
// stays zero and is never read: a whole copy of p would have its shape arrays indexed by a loop's counter, in scratch)
__device__ __forceinline__ SacView sac_pop_heads_view(const SacView &p, uint64_t key, const adc::SacLaw &law)
{
    SacView q{};
    q.sh.A = p.sh.A; q.sh.D = p.sh.D;
    q.update = p.update;
    q.key = key;
    q.law = law;
    return q;
}

// y of the element
template <bool NORM>
__global__ __launch_bounds__(kPgBlock) void k_sac_pop_target(SacView p, const MlpLearner *__restrict__ learners, const Td3Member *__restrict__ mem,
                                                             const SacMember *__restrict__ smem)
{
    extern __shared__ __align__(16) float sac_lds[];
    const Td3Member &me = mem[blockIdx.y];
    const MlpNet &pol = learners[blockIdx.y].net[0];
    const adc::Td3Shape &sh = p.sh;
    const adc::SacLaw law = smem[blockIdx.y].law;
    const uint64_t key = me.key;
    const int tid = threadIdx.x, D = sh.D;
    const uint32_t b = blockIdx.x;
    const Td3Ring ring = me.ring;
    const SacLds s = sac_carve(sac_lds, sh, p.maxw);
    const size_t slot = p.p_slot ? (size_t)p.p_slot[(size_t)blockIdx.y * gridDim.x + b] : (size_t)adc::td3_batch_index(key, b, p.update, p.size);
    const float alpha = smem[blockIdx.y].cell[kSacCellAlpha];
    const size_t nv = NORM ? (size_t)blockIdx.y * p.n_stride : 0;          // (the member's row of the normaliser's vectors; 0 whenever they are shared)
    // (the multiplier is read here, ahead of the networks' dependent rounds, not behind them where y is formed)
    const float r_mult = NORM && p.r_scale ? p.r_scale[(size_t)blockIdx.y * (size_t)p.r_stride] : 1.0f;
    for (int j = tid; j < D; j += kPgBlock) {
        float xj = ring.x2[slot * (size_t)D + j];
        if (NORM && p.n_shift) xj = adc::mlp_normalize(xj, p.n_shift[nv + j], p.n_scale[nv + j]);
        s.row[j] = xj;
    }
    __syncthreads();
    td3_forward(pol, sh.activation, s.row, s.yp, nullptr);
    sac_heads(sac_pop_heads_view(p, key, law), s, s.yp + adc::td3_hidden(sh.pol), adc::ST_SAC_NEXT, b);
    sac_lp(s, sh.A, s.words + 2);
    const int qlast = adc::td3_hidden(sh.q);
    for (int i = 0; i < 2; ++i) {
        td3_forward(me.q_t[i], sh.activation, s.row, s.yq, nullptr);
        if (tid == 0) s.words[i] = s.yq[qlast];
        __syncthreads();
    }
    if (tid == 0) {
        const float q = adc::td3_min(s.words[0], s.words[1]);
        p.ybuf[(size_t)blockIdx.y * gridDim.x + b] =
            NORM && p.r_scale ? adc::sac_y_norm(ring.r[slot], ring.done[slot], q, alpha, s.words[2], law, r_mult, p.r_clip)
                      : adc::sac_y(ring.r[slot], ring.done[slot], q, alpha, s.words[2], law);
    }
}

// forward and backward of both of the member's critics on the element, t = tanh(ring.a) as the action input
template <bool NORM>
__global__ __launch_bounds__(kPgBlock) void k_sac_pop_critic_sample(SacView p, const Td3Member *__restrict__ mem)
{
    extern __shared__ __align__(16) float sac_lds[];
    const adc::Td3Shape &sh = p.sh;
    const Td3Member &me = mem[blockIdx.y];
    const int tid = threadIdx.x, A = sh.A, D = sh.D, DA = D + A;
    const uint32_t b = blockIdx.x;
    const size_t at = (size_t)blockIdx.y * gridDim.x + b;       // the element's scratch row
    const Td3Ring ring = me.ring;
    const SacLds s = sac_carve(sac_lds, sh, p.maxw);
    const size_t slot = p.p_slot ? (size_t)p.p_slot[at] : (size_t)adc::td3_batch_index(me.key, b, p.update, p.size);
    float *xin = p.xin + at * (size_t)DA;
    const size_t nv = NORM ? (size_t)blockIdx.y * p.n_stride : 0;
    for (int j = tid; j < DA; j += kPgBlock) {
        float xj = j < D ? ring.x[slot * (size_t)D + j] : adc::mlp_tanh(ring.a[slot * (size_t)A + (j - D)]);
        if (NORM && p.n_shift && j < D) xj = adc::mlp_normalize(xj, p.n_shift[nv + j], p.n_scale[nv + j]);
        s.row[j] = xj;
        xin[j] = xj;
    }
    __syncthreads();
    const int nh = adc::td3_hidden(sh.q), no = adc::td3_outs(sh.q);
    float *acts = p.acts + at * (size_t)p.na, *deltas = p.deltas + at * (size_t)p.nd, *pc = p.pieces + at * adc::kTd3Pieces;
    for (int i = 0; i < 2; ++i) {
        td3_forward(me.q[i], sh.activation, s.row, s.yq, acts + i * nh);
        if (tid == 0) {
            const float y = p.ybuf[at], q = s.yq[nh];
            float loss;
            float d = adc::td3_critic_delta(q, y, loss);
            if (p.p_slot) { p.p_absd[2 * at + i] = __builtin_fabsf(d); d = p.p_w[at] * d; loss = p.p_w[at] * loss; }
            pc[adc::kTd3Loss1 + i] = loss; pc[adc::kTd3Q1 + i] = q;
            if (i == 0) { pc[adc::kTd3Y] = y; pc[adc::kSacPiLoss] = 0.0f; pc[adc::kSacLp] = 0.0f; pc[adc::kSacPick] = 0.0f; }
            s.d0[0] = d;
            deltas[i * no + nh] = d;
        }
        __syncthreads();
        td3_backward(me.q[i], sh.activation, s.yq, s.d0, s.d1, deltas + i * no, s.dump);
    }
}

// the member's actor forward and head, both of its critics on [x | t], the smaller one's backward through to the action inputs,
// the head's deltas for its 2A outputs, the actor's backward
template <bool NORM>
__global__ __launch_bounds__(kPgBlock) void k_sac_pop_actor_sample(SacView p, const MlpLearner *__restrict__ learners, const Td3Member *__restrict__ mem,
                                                                   const SacMember *__restrict__ smem)
{
    extern __shared__ __align__(16) float sac_lds[];
    const Td3Member &me = mem[blockIdx.y];
    const MlpNet &pol = learners[blockIdx.y].net[0];
    const adc::Td3Shape &sh = p.sh;
    const adc::SacLaw law = smem[blockIdx.y].law;
    const uint64_t key = me.key;
    const int tid = threadIdx.x, A = sh.A, D = sh.D;
    const uint32_t b = blockIdx.x;
    const size_t at = (size_t)blockIdx.y * gridDim.x + b;
    const SacLds s = sac_carve(sac_lds, sh, p.maxw);
    const size_t slot = p.p_slot ? (size_t)p.p_slot[(size_t)blockIdx.y * gridDim.x + b] : (size_t)adc::td3_batch_index(key, b, p.update, p.size);
    const float alpha = smem[blockIdx.y].cell[kSacCellAlpha];
    const float *rx = me.ring.x;
    const size_t nv = NORM ? (size_t)blockIdx.y * p.n_stride : 0;
    for (int j = tid; j < D; j += kPgBlock) {
        float xj = rx[slot * (size_t)D + j];
        if (NORM && p.n_shift) xj = adc::mlp_normalize(xj, p.n_shift[nv + j], p.n_scale[nv + j]);
        s.row[j] = xj;
    }
    __syncthreads();
    float *acts = p.acts + at * (size_t)p.na, *deltas = p.deltas + at * (size_t)p.nd;
    td3_forward(pol, sh.activation, s.row, s.yp, acts);
    const int ph = adc::td3_hidden(sh.pol), qh = adc::td3_hidden(sh.q), no = adc::td3_outs(sh.q);
    const float *o = s.yp + ph;
    sac_heads(sac_pop_heads_view(p, key, law), s, o, adc::ST_SAC_PI, b);
    sac_lp(s, A, s.words + 2);
    td3_forward(me.q[0], sh.activation, s.row, s.yq, nullptr);
    td3_forward(me.q[1], sh.activation, s.row, s.yq + no, nullptr);
    // the choice is the same in every lane: both values are read from LDS behind the layers' barrier
    const int pick = __builtin_amdgcn_readfirstlane(adc::sac_pick(s.yq[qh], s.yq[no + qh]));
    const float *yk = s.yq + pick * no;
    if (tid == 0) {
        float *pc = p.pieces + at * adc::kTd3Pieces;
        pc[adc::kSacPiLoss] = adc::sac_pi_loss(alpha, s.words[2], yk[qh]);
        pc[adc::kSacLp] = s.words[2];
        pc[adc::kSacPick] = (float)pick;
        s.d0[0] = 1.0f;
    }
    __syncthreads();
    // (pick is a scalar: the picked critic's layers are read from the member's row of the table at a uniform offset)
    const MlpNet &qn = me.q[pick];
    float *dq = td3_backward(qn, sh.activation, yk, s.d0, s.d1, nullptr, s.dump);
    float *dm = dq == s.d0 ? s.d1 : s.d0;
    // (td3_input_back leaves the negated input gradient: gq is its negation, exact)
    td3_input_back(qn.W[0], D, A, sh.q.n_out[0], dq, dm, nullptr, 0, s.gq);
    for (int a = tid; a < A; a += kPgBlock) {
        const float gq = -s.gq[a];
        const float du = adc::sac_du(s.row[D + a], s.w[a], gq, alpha, law.eps_sq);
        const float dls = adc::sac_dls(du, s.sd[a], s.z[a], alpha, adc::pg_clamp_moved(o[A + a], 1, law.ls_lo, law.ls_hi));
        dm[a] = du; dm[A + a] = dls;
        deltas[ph + a] = du; deltas[ph + A + a] = dls;
    }
    __syncthreads();
    td3_backward(pol, sh.activation, s.yp, dm, dq, deltas, s.dump);
}

// one step on every member's log_alpha from its joined sum of the actor step's lp (sums[member * sums_stride]); its cell follows.
// One lane per member; a member whose step has lr == 0 (alpha_lr == 0) writes nothing
__global__ void k_sac_pop_alpha(int M, const SacMember *__restrict__ smem, const double *__restrict__ sums, int sums_stride, long long B,
                                const Td3PopStep *__restrict__ steps)
{
    const int member = blockIdx.x * blockDim.x + threadIdx.x;
    if (member >= M) return;
    const adc::EsStep step = steps[member].step;
    if (!(step.lr > 0.0f)) return;
    float *cell = smem[member].cell;
    float m = cell[kSacCellM], v = cell[kSacCellV], alpha;
    const float la = adc::sac_alpha_step(step, cell[kSacCellLogAlpha],
                                         adc::sac_alpha_grad(sums[(size_t)member * (size_t)sums_stride], B, smem[member].target_entropy), m, v, alpha);
    cell[kSacCellLogAlpha] = la; cell[kSacCellM] = m; cell[kSacCellV] = v; cell[kSacCellAlpha] = alpha;
}
