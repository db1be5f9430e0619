// kernel_sac_pop.inc - SAC learner populations (adc_engine_sac_pop_*): M soft actor-critic learners in lock-step, every launch over
// all members.  The member is one more grid dimension, blockIdx.y, as in kernel_td3_pop.inc.  The target kernel is a wrapper
// of a few lines round the body its solo twin in kernel_sac.inc runs (sac_target_body): the body is written once, and a member's
// data enters through the wrapper's arguments alone; the critic and the actor kernel restate their solo twins' bodies
// (k_sac_critic_sample and k_sac_actor_sample say why).  What is a member's own is row blockIdx.y of the device tables
// MlpLearner[M] (its live actor), Td3Member[M] (its td3 key, its critics, target critics and ring; law.tau for Polyak; pol_t is not
// used) and SacMember[M] (its law constants, its target entropy, its temperature cell), and the member's index, which moves the
// scratch rows, ybuf, the pieces and the normaliser's vectors to the member's block.  The view p carries what the members share;
// p.law, p.pol, p.q, p.q_t, p.cell, p.ring and p.key are not read.  A member so runs the solo code on its own ring under its own
// key: its bits are a solo engine's, whatever M and the other members are.  Under a running normaliser (adc_sac_norm.h) the host
// launches the NORM = true instantiations; without one NORM = false, which does not read the normaliser's fields.  The store, the
// weight gradient, its join, the chunked sums, the optimiser step and Polyak are k_td3_pop_store / k_pg_pop_wgrad /
// k_pg_pop_grad_join / k_pg_pop_chunk_sums / k_pg_pop_join / k_td3_pop_step / k_td3_pop_polyak unchanged.  Td3PopStep[M] holds the
// next step's clip scale and optimiser constants.  All LDS is the dynamic region; no atomics; all stores are plain vector stores.
// (part of the single translation unit adc_engine.hip)
struct SacMember {
    adc::SacLaw law;
    float target_entropy;
    float *cell;                            // the member's {log_alpha, m, v, alpha}: its four floats of the [M][4] array
};

template <bool NORM>
__global__ __launch_bounds__(kPgBlock) void k_sac_pop_target(SacView p, const MlpLearner *__restrict__ learners, const Td3Member *__restrict__ mem,
                                                             const SacMember *__restrict__ smem)
{
    const Td3Member &me = mem[blockIdx.y];
    const SacMember &sm = smem[blockIdx.y];
    sac_target_body<NORM>(p, learners[blockIdx.y].net[0], me.q_t, sm.law, me.key, me.ring, sm.cell, blockIdx.y);
}

// k_sac_critic_sample restated for member blockIdx.y (see there why the two do not share a body): forward and backward of both of
// the member's critics on the element, t = tanh(ring.a) as the action input
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

// k_sac_actor_sample restated for member blockIdx.y (see there why the two do not share a body): the member's actor forward and
// head, both of its critics on [x | t], the smaller one's backward through to the action inputs, the head's deltas for its 2A
// outputs, the actor's backward.  The scratch rows and pieces start at member * gridDim.x, the normaliser's vectors at
// member * p.n_stride
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
    sac_heads(A, D, p.update, key, law, s, o, adc::ST_SAC_PI, b);
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
// One lane per member; a member whose step has lr == 0 (alpha_lr == 0) writes nothing.  (k_sac_alpha's arithmetic in another shape -
// a lane per member, the lr test - so the two are not one body)
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
