// kernel_td3_pop.inc - TD3 learner populations (adc_engine_td3_pop_*): M off-policy learners in lock-step, every launch over all
// members.  The member is one more grid dimension, blockIdx.y.  Every kernel here but the critics' is a wrapper of a few lines round
// the body its solo twin in kernel_td3.inc runs (td3_store_body, td3_target_body, td3_actor_body, td3_polyak_body;
// pg_pop_update_body of kernel_pg.inc for the optimiser step; k_td3_pop_critic_sample restates k_td3_critic_sample, which says
// why): the body is written once, and a member's data enters through the
// wrapper's arguments alone - row blockIdx.y of the device tables MlpLearner[M] (its live actor), Td3Member[M] (its law constants,
// its td3 key, its critics, targets and ring) and Td3PopStep[M] (the next step's clip scale and optimiser constants), and the
// member's index, which moves the scratch rows and the normaliser's vectors to the member's block.  The view p carries what the
// members share; p.pol, p.pol_t, p.q, p.q_t, p.law, p.key and p.ring are not read.  A member so runs the solo code on its own
// ring under its own key: its bits are a solo engine's, whatever M and the other members are.  The weight gradient, its join and
// the chunked sums are k_pg_pop_wgrad / k_pg_pop_grad_join / k_pg_pop_chunk_sums / k_pg_pop_join unchanged.  All LDS is the
// dynamic region; no atomics; all stores are plain vector stores.
// (part of the single translation unit adc_engine.hip)
struct Td3Member {
    adc::Td3Law law;
    uint64_t key;
    MlpNet pol_t, q[2], q_t[2];             // the member's own chain-major stores (its live actor is MlpLearner::net[0])
    Td3Ring ring;                           // its C slots
};

// one member's next optimiser step: clip on / off, the clip's scale, the step's constants (its bias corrections included)
struct Td3PopStep {
    int clip;
    float scale;
    adc::EsStep step;
};

__global__ __launch_bounds__(kPgBlock) void k_td3_pop_store(View v, const float *__restrict__ shift, const float *__restrict__ scale, int D, int A,
                                                            const float *__restrict__ ro_obs, const float *__restrict__ ro_action,
                                                            const float *__restrict__ ro_reward, const uint8_t *__restrict__ ro_term,
                                                            const uint8_t *__restrict__ ro_trunc, int t0, int t1, int envs_per_member,
                                                            const Td3Member *__restrict__ mem, unsigned long long written, unsigned long long C)
{
    td3_store_body(v, shift, scale, D, A, ro_obs, ro_action, ro_reward, ro_term, ro_trunc, t0, t1, envs_per_member, blockIdx.y, mem[blockIdx.y].ring,
                   written, C);
}
// ... with an observation history (adc_engine_mlp_init_frames, frames > 1)
__global__ __launch_bounds__(kPgBlock) void k_td3_pop_store_hist(View v, const float *__restrict__ shift, const float *__restrict__ scale, int D, int A,
                                                                 const float *__restrict__ ro_obs, const float *__restrict__ ro_action,
                                                                 const float *__restrict__ ro_reward, const uint8_t *__restrict__ ro_term,
                                                                 const uint8_t *__restrict__ ro_trunc, int t0, int t1, int envs_per_member,
                                                                 const Td3Member *__restrict__ mem, unsigned long long written, unsigned long long C,
                                                                 const float *__restrict__ hist, const int32_t *__restrict__ h_last,
                                                                 const int32_t *__restrict__ h_from, int frames)
{
    td3_store_body<true>(v, shift, scale, D, A, ro_obs, ro_action, ro_reward, ro_term, ro_trunc, t0, t1, envs_per_member, blockIdx.y,
                         mem[blockIdx.y].ring, written, C, hist, h_last, h_from, frames);
}

// ... with n-step returns (adc_engine_replay_nstep_init): every member's window under its own law.gamma (a SAC member's Td3Member
// carries its gamma too)
__global__ __launch_bounds__(kPgBlock) void k_td3_pop_store_nstep(View v, const float *__restrict__ shift, const float *__restrict__ scale, int D, int A,
                                                                  const float *__restrict__ ro_obs, const float *__restrict__ ro_action,
                                                                  const float *__restrict__ ro_reward, const uint8_t *__restrict__ ro_term,
                                                                  const uint8_t *__restrict__ ro_trunc, int t0, int t1, int envs_per_member,
                                                                  const Td3Member *__restrict__ mem, unsigned long long written,
                                                                  unsigned long long C, int nstep)
{
    td3_store_body<false, true>(v, shift, scale, D, A, ro_obs, ro_action, ro_reward, ro_term, ro_trunc, t0, t1, envs_per_member, blockIdx.y,
                                mem[blockIdx.y].ring, written, C, nullptr, nullptr, nullptr, 1, nstep, mem[blockIdx.y].law.gamma);
}
__global__ __launch_bounds__(kPgBlock) void k_td3_pop_store_hist_nstep(View v, const float *__restrict__ shift, const float *__restrict__ scale, int D,
                                                                       int A, const float *__restrict__ ro_obs, const float *__restrict__ ro_action,
                                                                       const float *__restrict__ ro_reward, const uint8_t *__restrict__ ro_term,
                                                                       const uint8_t *__restrict__ ro_trunc, int t0, int t1, int envs_per_member,
                                                                       const Td3Member *__restrict__ mem, unsigned long long written,
                                                                       unsigned long long C, const float *__restrict__ hist,
                                                                       const int32_t *__restrict__ h_last, const int32_t *__restrict__ h_from,
                                                                       int frames, int nstep)
{
    td3_store_body<true, true>(v, shift, scale, D, A, ro_obs, ro_action, ro_reward, ro_term, ro_trunc, t0, t1, envs_per_member, blockIdx.y,
                               mem[blockIdx.y].ring, written, C, hist, h_last, h_from, frames, nstep, mem[blockIdx.y].law.gamma);
}

__global__ __launch_bounds__(kPgBlock) void k_td3_pop_target(Td3View p, const Td3Member *__restrict__ mem)
{
    const Td3Member &me = mem[blockIdx.y];
    td3_target_body(p, me.pol_t, me.q_t, me.law, me.key, me.ring, blockIdx.y);
}
__global__ __launch_bounds__(kPgBlock) void k_td3_pop_target_bounded(Td3View p, const Td3Member *__restrict__ mem)
{
    const Td3Member &me = mem[blockIdx.y];
    td3_target_body<true>(p, me.pol_t, me.q_t, me.law, me.key, me.ring, blockIdx.y);
}

// k_td3_critic_sample restated for member blockIdx.y (see there why the two do not share a body): forward and backward of both of
// the member's critics on the element; the scratch rows start at member * gridDim.x, the normaliser's vectors at member * p.n_stride
__global__ __launch_bounds__(kPgBlock) void k_td3_pop_critic_sample(Td3View p, const Td3Member *__restrict__ mem)
{
    extern __shared__ __align__(16) float td3_lds[];
    const adc::Td3Shape &sh = p.sh;
    const Td3Member &me = mem[blockIdx.y];
    const int tid = threadIdx.x, A = sh.A, D = sh.D, DA = D + A;
    const uint32_t b = blockIdx.x;
    const size_t at = (size_t)blockIdx.y * gridDim.x + b;       // the element's scratch row
    const Td3Ring ring = me.ring;
    float *row = td3_lds, *yq = row + DA + adc::td3_outs(sh.pol), *d0 = yq + adc::td3_outs(sh.q), *d1 = d0 + p.maxw, *dump = d1 + p.maxw;
    const size_t slot = p.p_slot ? (size_t)p.p_slot[at] : (size_t)adc::td3_batch_index(me.key, b, p.update, p.size);
    float *xin = p.xin + at * (size_t)DA;
    const size_t nv = (size_t)blockIdx.y * p.n_stride;
    for (int j = tid; j < DA; j += kPgBlock) {
        float xj = j < D ? ring.x[slot * (size_t)D + j]
                         : adc::td3_action_norm(ring.a[slot * (size_t)A + (j - D)], p.a_shift, p.a_scale, j - D, sh.norm);
        if (p.n_shift && j < D) xj = adc::mlp_normalize(xj, p.n_shift[nv + j], p.n_scale[nv + j]);
        row[j] = xj;
        xin[j] = xj;
    }
    __syncthreads();
    const int nh = adc::td3_hidden(sh.q), no = adc::td3_outs(sh.q);
    float *acts = p.acts + at * (size_t)p.na, *deltas = p.deltas + at * (size_t)p.nd, *pc = p.pieces + at * adc::kTd3Pieces;
    for (int i = 0; i < 2; ++i) {
        td3_forward(me.q[i], sh.activation, row, yq, acts + i * nh);
        if (tid == 0) {
            const float y = p.ybuf[at], q = yq[nh];
            float loss;
            float d = adc::td3_critic_delta(q, y, loss);
            if (p.p_slot) { p.p_absd[2 * at + i] = __builtin_fabsf(d); d = p.p_w[at] * d; loss = p.p_w[at] * loss; }
            pc[adc::kTd3Loss1 + i] = loss; pc[adc::kTd3Q1 + i] = q;
            if (i == 0) { pc[adc::kTd3Y] = y; pc[adc::kTd3QPi] = 0.0f; pc[6] = 0.0f; pc[7] = 0.0f; }
            d0[0] = d;
            deltas[i * no + nh] = d;
        }
        __syncthreads();
        td3_backward(me.q[i], sh.activation, yq, d0, d1, deltas + i * no, dump);
    }
}

__global__ __launch_bounds__(kPgBlock) void k_td3_pop_actor_sample(Td3View p, const MlpLearner *__restrict__ learners, const Td3Member *__restrict__ mem)
{
    const Td3Member &me = mem[blockIdx.y];
    td3_actor_body(p, learners[blockIdx.y].net[0], me.q[0], me.key, me.ring, blockIdx.y);
}
__global__ __launch_bounds__(kPgBlock) void k_td3_pop_actor_sample_bounded(Td3View p, const MlpLearner *__restrict__ learners,
                                                                           const Td3Member *__restrict__ mem)
{
    const Td3Member &me = mem[blockIdx.y];
    td3_actor_body<true>(p, learners[blockIdx.y].net[0], me.q[0], me.key, me.ring, blockIdx.y);
}

// the (clipped) gradient's step of every member with its own clip scale and step constants: k_pg_pop_update on a Td3PopStep row
__global__ __launch_bounds__(kPgBlock) void k_td3_pop_step(PgLayout L, size_t stride, float *__restrict__ theta, float *__restrict__ mom_m,
                                                           float *__restrict__ mom_v, const float *__restrict__ grad,
                                                           const Td3PopStep *__restrict__ steps)
{
    pg_pop_update_body(L, stride, theta, mom_m, mom_v, grad, steps);
}

// Polyak with the member's tau on the [M][Q] vectors
__global__ __launch_bounds__(kPgBlock) void k_td3_pop_polyak(PgLayout L, size_t stride, float *__restrict__ target, const float *__restrict__ param,
                                                             const Td3Member *__restrict__ mem)
{
    td3_polyak_body(L, stride, target, param, mem[blockIdx.y].law.tau, blockIdx.y);
}
