// kernel_td3_pop.inc - TD3 learner populations (adc_engine_td3_pop_*): M off-policy learners in lock-step, every launch over all
// members.  The member is one more grid dimension: what is a member's own is read from the device tables MlpLearner[M] (its live
// actor), Td3Member[M] (its law constants, its td3 key, its critics, targets and ring) and Td3PopStep[M] (the next step's clip
// scale and optimiser constants), and the member's batch, scratch rows and partials are the solo kernel's with a base moved to the
// member's block.  The arithmetic is adc_td3.h's law through the same helpers kernel_td3.inc uses (td3_forward, td3_backward,
// td3_input_back): a member runs the solo code on its own ring under its own key, so its bits are a solo engine's, whatever M
// and the other members are.  The three batch kernels restate the solo kernels' bodies rather than share them: kernel_td3.inc and
// its bodies stay the solo learner's alone.  The weight gradient, its join and the chunked sums are k_pg_pop_wgrad /
// k_pg_pop_grad_join / k_pg_pop_chunk_sums / k_pg_pop_join unchanged.  All LDS is the dynamic region; no atomics; all stores are
// plain vector stores.
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

// sample s = (t - t0) * n + local env of member blockIdx.y's envs [member n, (member + 1) n) into its slot (written + s) mod C
__global__ __launch_bounds__(kPgBlock) void k_td3_pop_store(View v, const float *__restrict__ shift, const float *__restrict__ scale, int D, int A,
                                                            const float *__restrict__ ro_obs, const float *__restrict__ ro_action,
                                                            const float *__restrict__ ro_reward, const uint8_t *__restrict__ ro_term,
                                                            const uint8_t *__restrict__ ro_trunc, int t0, int t1, int envs_per_member,
                                                            const Td3Member *__restrict__ mem, unsigned long long written, unsigned long long C)
{
    const int tid = threadIdx.x, N = v.N, K = v.K, n = envs_per_member, member = blockIdx.y;
    const unsigned long long s = blockIdx.x, count = (unsigned long long)(t1 - t0) * (unsigned long long)n;
    if (s >= count || s + C < count) return;            // (a later sample of this store lands on the same slot)
    const int t = t0 + (int)(s / (unsigned long long)n), env = member * n + (int)(s % (unsigned long long)n);
    const Td3Ring ring = mem[member].ring;
    const size_t slot = (size_t)((written + s) % C), row = (size_t)t * (size_t)N + (size_t)env;
    for (int j = tid; j < D; j += kPgBlock) ring.x[slot * (size_t)D + j] = ro_obs[row * (size_t)D + j];
    for (int a = tid; a < A; a += kPgBlock) ring.a[slot * (size_t)A + a] = ro_action[row * (size_t)A + a];
    if (tid == 0) {
        ring.r[slot] = ro_reward[row];
        ring.done[slot] = (uint8_t)((ro_term[row] | ro_trunc[row]) ? 1 : 0);
    }
    if (t + 1 < t1) {
        const size_t next = row + (size_t)N;
        for (int j = tid; j < D; j += kPgBlock) ring.x2[slot * (size_t)D + j] = ro_obs[next * (size_t)D + j];
    } else {
        // the input row an act would read now (k_mlp_policy's prologue)
        const bool first = v.day[env] == 0;
        const size_t o = (size_t)env * K;
        const double cum = v.cum_profit[env];
        const int32_t days = v.day_out[env];
        for (int j = tid; j < D; j += kPgBlock) {
            float xj = first ? 0.0f : adc::mlp_obs_at(j, K, v.clk + o, v.cost + o, v.imp + o, v.rev + o, v.conv + o, cum, days);
            if (shift) xj = adc::mlp_normalize(xj, shift[j], scale[j]);
            ring.x2[slot * (size_t)D + j] = xj;
        }
    }
}

// The batch kernels: batch element blockIdx.x of member blockIdx.y.  p carries what the members share (the shapes, the action
// normalisation, the ring's size, the update's number, the scratch for all members, na / nd / maxw); p.pol, p.pol_t, p.q, p.q_t,
// p.law, p.key and p.ring are not read.  A member's scratch rows start at member * gridDim.x.  Under a running normaliser
// (p.n_shift / p.r_scale non-null) the member's vectors are at member * p.n_stride, its multiplier at member * p.r_stride.

// y of the element
__global__ __launch_bounds__(kPgBlock) void k_td3_pop_target(Td3View p, const Td3Member *__restrict__ mem)
{
    extern __shared__ __align__(16) float td3_lds[];
    const adc::Td3Shape &sh = p.sh;
    const Td3Member &me = mem[blockIdx.y];
    const int tid = threadIdx.x, A = sh.A, D = sh.D;
    const uint32_t b = blockIdx.x;
    const uint64_t key = me.key;
    const Td3Ring ring = me.ring;
    float *row = td3_lds, *yp = row + D + A, *yq = yp + adc::td3_outs(sh.pol), *words = yq + adc::td3_outs(sh.q) + 3 * p.maxw;
    const size_t slot = p.p_slot ? (size_t)p.p_slot[(size_t)blockIdx.y * gridDim.x + b] : (size_t)adc::td3_batch_index(key, b, p.update, p.size);
    const size_t nv = (size_t)blockIdx.y * p.n_stride;          // (the member's row of the normaliser's vectors; 0 whenever they are shared)
    // (the multiplier is read here, ahead of the networks' dependent rounds, not behind them where y is formed)
    const float r_mult = p.r_scale ? p.r_scale[(size_t)blockIdx.y * (size_t)p.r_stride] : 1.0f;
    for (int j = tid; j < D; j += kPgBlock) {
        float xj = ring.x2[slot * (size_t)D + j];
        if (p.n_shift) xj = adc::mlp_normalize(xj, p.n_shift[nv + j], p.n_scale[nv + j]);
        row[j] = xj;
    }
    __syncthreads();
    td3_forward(me.pol_t, sh.activation, row, yp, nullptr);
    const float *mu = yp + adc::td3_hidden(sh.pol);
    const adc::Td3Law law = me.law;
    for (int a = tid; a < A; a += kPgBlock) {
        const float ap = adc::td3_target_action(mu[a], adc::td3_noise(key, a, b, p.update), law);
        row[D + a] = adc::td3_action_norm(ap, p.a_shift, p.a_scale, a, sh.norm);
    }
    __syncthreads();
    const int qlast = adc::td3_hidden(sh.q);
    for (int i = 0; i < 2; ++i) {
        td3_forward(me.q_t[i], sh.activation, row, yq, nullptr);
        if (tid == 0) words[i] = yq[qlast];
        __syncthreads();
    }
    if (tid == 0) {
        const float q = adc::td3_min(words[0], words[1]);
        p.ybuf[(size_t)blockIdx.y * gridDim.x + b] =
            p.r_scale ? adc::td3_y_norm(ring.r[slot], ring.done[slot], q, law, r_mult, p.r_clip)
                      : adc::td3_y(ring.r[slot], ring.done[slot], q, law);
    }
}

// forward and backward of both of the member's critics on the element
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

// the member's actor forward, its critic 1 on [x | norm(mu)], the backward through to the action inputs, the actor's backward
__global__ __launch_bounds__(kPgBlock) void k_td3_pop_actor_sample(Td3View p, const MlpLearner *__restrict__ learners, const Td3Member *__restrict__ mem)
{
    extern __shared__ __align__(16) float td3_lds[];
    const adc::Td3Shape &sh = p.sh;
    const Td3Member &me = mem[blockIdx.y];
    const MlpNet &pol = learners[blockIdx.y].net[0];
    const int tid = threadIdx.x, A = sh.A, D = sh.D;
    const uint32_t b = blockIdx.x;
    const size_t at = (size_t)blockIdx.y * gridDim.x + b;
    float *row = td3_lds, *yp = row + D + A, *yq = yp + adc::td3_outs(sh.pol), *d0 = yq + adc::td3_outs(sh.q), *d1 = d0 + p.maxw, *dump = d1 + p.maxw;
    const size_t slot = p.p_slot ? (size_t)p.p_slot[at] : (size_t)adc::td3_batch_index(me.key, b, p.update, p.size);
    const float *rx = me.ring.x;
    const size_t nv = (size_t)blockIdx.y * p.n_stride;
    for (int j = tid; j < D; j += kPgBlock) {
        float xj = rx[slot * (size_t)D + j];
        if (p.n_shift) xj = adc::mlp_normalize(xj, p.n_shift[nv + j], p.n_scale[nv + j]);
        row[j] = xj;
    }
    __syncthreads();
    float *acts = p.acts + at * (size_t)p.na, *deltas = p.deltas + at * (size_t)p.nd;
    td3_forward(pol, sh.activation, row, yp, acts);
    const int ph = adc::td3_hidden(sh.pol), qh = adc::td3_hidden(sh.q);
    for (int a = tid; a < A; a += kPgBlock) row[D + a] = adc::td3_action_norm(yp[ph + a], p.a_shift, p.a_scale, a, sh.norm);
    __syncthreads();
    td3_forward(me.q[0], sh.activation, row, yq, nullptr);
    if (tid == 0) {
        p.pieces[at * adc::kTd3Pieces + adc::kTd3QPi] = yq[qh];
        d0[0] = 1.0f;
    }
    __syncthreads();
    float *dq = td3_backward(me.q[0], sh.activation, yq, d0, d1, nullptr, dump);
    float *dm = dq == d0 ? d1 : d0;
    td3_input_back(me.q[0].W[0], D, A, sh.q.n_out[0], dq, dm, p.a_scale, sh.norm, deltas + ph);
    td3_backward(pol, sh.activation, yp, dm, dq, deltas, dump);
}

// the (clipped) gradient's step of every member (blockIdx.y) with its own clip scale and step constants; theta, the moments and grad
// are [M][Q], L member 0's stores and a member's `stride` floats further each
__global__ __launch_bounds__(kPgBlock) void k_td3_pop_step(PgLayout L, size_t stride, float *__restrict__ theta, float *__restrict__ mom_m,
                                                           float *__restrict__ mom_v, const float *__restrict__ grad,
                                                           const Td3PopStep *__restrict__ steps)
{
    const int p = blockIdx.x * kPgBlock + threadIdx.x;
    if (p >= L.Q) return;
    const size_t member = blockIdx.y, i = member * (size_t)L.Q + (size_t)p;
    const Td3PopStep &c = steps[member];
    float g = grad[i];
    if (c.clip) g = g * c.scale;
    float m = mom_m[i], v = mom_v[i];
    const float t1 = adc::pg_apply(c.step, theta[i], g, m, v);
    theta[i] = t1;
    mom_m[i] = m;
    mom_v[i] = v;
    *(pg_param_slot(L, p) + member * stride) = t1;
}

// target = target + tau * (param - target) with the member's tau on the [M][Q] vectors, the targets' chain-major stores rebuilt
__global__ __launch_bounds__(kPgBlock) void k_td3_pop_polyak(PgLayout L, size_t stride, float *__restrict__ target, const float *__restrict__ param,
                                                             const Td3Member *__restrict__ mem)
{
    const int p = blockIdx.x * kPgBlock + threadIdx.x;
    if (p >= L.Q) return;
    const size_t member = blockIdx.y, i = member * (size_t)L.Q + (size_t)p;
    const float t1 = adc::td3_polyak(target[i], param[i], mem[member].law.tau);
    target[i] = t1;
    *(pg_param_slot(L, p) + member * stride) = t1;
}
