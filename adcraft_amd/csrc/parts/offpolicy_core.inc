// offpolicy_core.inc - the host side that the four off-policy front ends share (td3_api.inc, sac_api.inc, td3_pop_api.inc,
// sac_pop_api.inc): the replay ring's fetch / load / copy, the critic upload, the batch indices, the store's refusals and
// bookkeeping, the state vectors, the allocation, the launch helpers of an update and the populations' update driver.  All four
// live in the same engine fields (host_api.inc: td3_*, tp_*, sp_*).  `member` is a population's member, or kOffSolo for the
// single-learner trainers (their ring is e->td3_ring, their stores td3_lay's, their critic flags td3_critic_set).  A function here
// that refuses arguments takes ENGINE_GUARD itself, after its refusals: a refused call leaves the env groups as they were.
// (part of the single translation unit adc_engine.hip)
namespace {
// prioritised replay's side of an update, a store, a buffer load and a member copy (parts/per_api.inc; called only while e->per_live)
int per_sample_run(adc_engine *e, uint32_t update);
int per_leaves_run(adc_engine *e);
int per_store_run(adc_engine *e, int64_t written_before, int64_t count);
int per_loaded_run(adc_engine *e, int member, int64_t slot, int64_t count);
int per_copy_run(adc_engine *e, int src, int dst);
void per_pairs_launch(adc_engine *e, int npairs);
enum { kTd3Theta = 0, kTd3Psi = 1, kTd3ThetaT = 2, kTd3PsiT = 3 };
constexpr int kOffSolo = -1;
inline size_t off_m(int member) { return member < 0 ? 0 : (size_t)member; }
constexpr size_t kOffCriticFlags = 2u * adc::kMlpMaxLayers;         // tp_critic_set's entries per member

inline int64_t td3_size(const adc_engine *e) { return std::min<int64_t>(e->td3_written, (int64_t)e->td3_cfg.capacity); }
inline size_t tp_count(const adc_engine *e, int which) { return (which & 1) ? 2 * (size_t)e->td3_Qc : (size_t)e->td3_P; }
inline const Td3Ring &off_ring(const adc_engine *e, int member) { return member < 0 ? e->td3_ring : e->tp_mem[(size_t)member].ring; }
int tp_member_check(const adc_engine *e, int32_t member)
{
    if (member < 0 || member >= e->lrn_M) return fail(ADC_EINVAL, "no such member");
    return ADC_OK;
}

// ---- flat vectors against the chain-major stores (the flat order is flat_layout of parts/mlp_core.inc) -----------------------------
// the critics', the target actor's (none: SAC) and the target critics' flat orders; theta's is the front end's
void off_layouts(adc_engine *e, const MlpNet *q, const MlpNet *q_t, const MlpNet &pol_t)
{
    e->td3_lay[kTd3Psi] = flat_layout(q, 2);
    e->td3_lay[kTd3ThetaT] = pol_t.layers ? flat_layout(&pol_t, 1) : PgLayout{};
    e->td3_lay[kTd3PsiT] = flat_layout(q_t, 2);
}
// a population's theta: the learners' policy layers; the other vectors' stores are `stride` floats apart
void tp_theta_layout(adc_engine *e, size_t stride)
{
    e->td3_lay[kTd3Theta] = e->lrn_lay;
    e->td3_lay[kTd3Theta].nterms = e->td3_shape.pol.layers; e->td3_lay[kTd3Theta].Q = e->td3_P;
    e->tp_stride[kTd3Theta] = e->lrn_stride;
    e->tp_stride[kTd3Psi] = e->tp_stride[kTd3ThetaT] = e->tp_stride[kTd3PsiT] = stride;
}
// which = 1: flat <- stores; 0: stores <- flat
void td3_params_copy(adc_engine *e, int which, int to_flat)
{
    const PgLayout &lay = e->td3_lay[which];
    hipLaunchKernelGGL(k_pg_params_copy, dim3((unsigned)((lay.Q + kPgBlock - 1) / kPgBlock)), dim3(kPgBlock), 0, e->stream, lay, e->td3_flat[which], to_flat);
}
// the members member0 .. member0 + count - 1: flat <- stores (to_flat) or stores <- flat, of vector `which`
void tp_params_copy(adc_engine *e, int which, int member0, int count, int to_flat)
{
    const PgLayout &lay = e->td3_lay[which];
    const size_t Q = tp_count(e, which);
    hipLaunchKernelGGL(k_pg_pop_params_copy, dim3(pg_blocks(lay.Q), (unsigned)count), dim3(kPgBlock), 0, e->stream, lay, e->tp_stride[which], member0,
                       e->td3_flat[which] + (size_t)member0 * Q, Q, to_flat);
}
void off_params_copy(adc_engine *e, int which, int member0, int count, int to_flat)
{
    if (member0 < 0) td3_params_copy(e, which, to_flat);
    else tp_params_copy(e, which, member0, count, to_flat);
}
// the targets of `count` members from member0 on (or the solo trainer's) become copies: of the actor and the critics
// (first = 0: TD3) or of the critics alone (first = 1: SAC has no target actor)
int off_sync_run(adc_engine *e, int member0, int count, int first)
{
    for (int w = first; w < 2; ++w) {
        const size_t Q = tp_count(e, w), at = off_m(member0) * Q;
        HIP_TRY(hipMemcpyAsync(e->td3_flat[kTd3ThetaT + w] + at, e->td3_flat[kTd3Theta + w] + at, (size_t)count * Q * 4, hipMemcpyDeviceToDevice, e->stream));
        off_params_copy(e, kTd3ThetaT + w, member0, count, 0);
    }
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}

// ---- the critics' upload -------------------------------------------------------------------------------------------------------
inline bool off_critic_flag(const adc_engine *e, int member, int critic, int layer)
{
    return member < 0 ? e->td3_critic_set[critic][layer] : e->tp_critic_set[(size_t)member * kOffCriticFlags + (size_t)critic * adc::kMlpMaxLayers + (size_t)layer] != 0;
}
// every critic layer of the solo trainer (pop = false) or of every member has been uploaded
bool off_critics_set(const adc_engine *e, bool pop)
{
    for (int m = 0; m < (pop ? e->lrn_M : 1); ++m)
        for (int i = 0; i < 2; ++i)
            for (int l = 0; l < e->td3_shape.q.layers; ++l)
                if (!off_critic_flag(e, pop ? m : kOffSolo, i, l)) return false;
    return true;
}
// (a state vector carries every layer)
void off_critics_mark(adc_engine *e, int member)
{
    if (member < 0) {
        for (int i = 0; i < 2; ++i)
            for (int l = 0; l < e->td3_shape.q.layers; ++l) e->td3_critic_set[i][l] = true;
    } else
        for (size_t i = 0; i < kOffCriticFlags; ++i) e->tp_critic_set[(size_t)member * kOffCriticFlags + i] = 1;
}
int off_set_critic_layer(adc_engine *e, int member, int32_t critic, int32_t layer, const float *weights_in_out, const float *bias_out)
{
    if (critic != 0 && critic != 1) return fail(ADC_EINVAL, "critic: 0 or 1");
    const adc::Td3Net &q = e->td3_shape.q;
    if (layer < 0 || layer >= q.layers) return fail(ADC_EINVAL, "no such critic layer");
    if (!weights_in_out || !bias_out) return fail(ADC_EINVAL, "weights or bias is NULL");
    ENGINE_GUARD(e);
    size_t off = off_m(member) * 2u * (size_t)e->td3_Qc + (size_t)critic * (size_t)e->td3_Qc;
    for (int l = 0; l < layer; ++l) off += (size_t)(adc::td3_n_in(q, l) + 1) * (size_t)q.n_out[l];
    const size_t nw = (size_t)adc::td3_n_in(q, layer) * (size_t)q.n_out[layer];
    HIP_TRY(hipMemcpyAsync(e->td3_flat[kTd3Psi] + off, weights_in_out, nw * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->td3_flat[kTd3Psi] + off + nw, bias_out, (size_t)q.n_out[layer] * 4, hipMemcpyHostToDevice, e->stream));
    off_params_copy(e, kTd3Psi, member, 1, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (member < 0) e->td3_critic_set[critic][layer] = true;
    else e->tp_critic_set[(size_t)member * kOffCriticFlags + (size_t)critic * adc::kMlpMaxLayers + (size_t)layer] = 1;
    return ADC_OK;
}

// ---- the replay ring -----------------------------------------------------------------------------------------------------------
// the act and a TD3 learner agree on the action's units (adc_td3.h "bounded"): checked at every store and update of the TD3 front ends
int td3_bounded_check(const adc_engine *e, const adc_td3_config *cfgs, size_t count)
{
    if (!e->td3_bounded) {
        if (e->mp.bd_lo) return fail(ADC_ESTATE, "the act is bounded: its actions are in units of the box, and the learner must be bounded too (adc_engine_td3_set_bounded / adc_engine_td3_pop_set_bounded)");
        return ADC_OK;
    }
    if (!e->mp.bd_lo) return fail(ADC_ESTATE, "bounded TD3 needs the bounded act (adc_engine_mlp_set_bounds, or adc_engine_mlp_learners_set_bounds for a population)");
    for (size_t m = 0; m < count; ++m)
        if (cfgs[m].action_hi > cfgs[m].action_lo)
            return fail(ADC_ESTATE, "bounded TD3 with action_lo / action_hi set is not supported: the target action's box is [-1, 1]");
    return ADC_OK;
}
int off_store_check(const adc_engine *e)
{
    if (e->ro_t <= e->td3_stored_t) return fail(ADC_ESTATE, "no unstored day in the record (adc_engine_mlp_step / adc_engine_run_days with ADC_POLICY_MLP)");
    if (e->td3_gap || e->env_moves != e->ro_moves)
        return fail(ADC_ESTATE, "the envs were stepped or reset outside the record since an unstored recorded day: its next observation is not the "
                                "one the envs hold (adc_engine_rollout_reset, collect again)");
    return ADC_OK;
}
// a front end's store launch under n-step returns (adc_engine_replay_nstep_init; adc_td3.h "n-step"): `count` samples per member,
// pop: over every member's ring under its own gamma; raw: the learners' observation normaliser is alive, the rows stay raw
void off_store_nstep_launch(adc_engine *e, bool pop, bool raw, long long count)
{
    const float *shift = raw ? nullptr : e->mp.shift, *scale = raw ? nullptr : e->mp.scale;
    const unsigned long long written = (unsigned long long)e->td3_written, C = (unsigned long long)e->td3_cfg.capacity;
    const bool hist = e->mp.frames > 1;
    if (pop && hist)
        hipLaunchKernelGGL(k_td3_pop_store_hist_nstep, dim3((unsigned)count, (unsigned)e->lrn_M), dim3(kPgBlock), 0, e->stream, e->v, shift, scale, e->mp.D,
                           e->mp.A, e->ro_obs, e->ro_action, e->ro_reward, e->ro_term, e->ro_trunc, e->td3_stored_t, e->ro_t, e->lrn_n, e->tp_dmem, written, C,
                           e->mp.hist, e->mp.last, e->mp.from, e->mp.frames, e->nstep_n);
    else if (pop)
        hipLaunchKernelGGL(k_td3_pop_store_nstep, dim3((unsigned)count, (unsigned)e->lrn_M), dim3(kPgBlock), 0, e->stream, e->v, shift, scale, e->mp.D, e->mp.A,
                           e->ro_obs, e->ro_action, e->ro_reward, e->ro_term, e->ro_trunc, e->td3_stored_t, e->ro_t, e->lrn_n, e->tp_dmem, written, C,
                           e->nstep_n);
    else if (hist)
        hipLaunchKernelGGL(k_td3_store_hist_nstep, dim3((unsigned)count), dim3(kPgBlock), 0, e->stream, e->v, shift, scale, e->mp.D, e->mp.A, e->ro_obs,
                           e->ro_action, e->ro_reward, e->ro_term, e->ro_trunc, e->td3_stored_t, e->ro_t, e->td3_ring, written, C, e->mp.hist, e->mp.last,
                           e->mp.from, e->mp.frames, e->nstep_n, e->td3_cfg.gamma);
    else
        hipLaunchKernelGGL(k_td3_store_nstep, dim3((unsigned)count), dim3(kPgBlock), 0, e->stream, e->v, shift, scale, e->mp.D, e->mp.A, e->ro_obs,
                           e->ro_action, e->ro_reward, e->ro_term, e->ro_trunc, e->td3_stored_t, e->ro_t, e->td3_ring, written, C, e->nstep_n,
                           e->td3_cfg.gamma);     // (a solo SAC learner's gamma is td3_cfg's too: sac_as_td3)
}
// after the front end's store launch of `count` transitions (per member): the ring's counters move
int off_store_done(adc_engine *e, long long count, int64_t *stored)
{
    HIP_TRY(hipGetLastError());
    if (e->per_live)
        if (int rc = per_store_run(e, e->td3_written, count)) return rc;
    e->td3_written += count;
    e->td3_stored_t = e->ro_t;
    if (stored) *stored = count;
    return ADC_OK;
}
// (batch_size: the populations' buffer_info alone has it; the solo trainers have a *_batch_size entry point)
int off_buffer_info(const adc_engine *e, int64_t *size, int64_t *written, int64_t *capacity, int32_t *batch_size)
{
    if (size) *size = td3_size(e);
    if (written) *written = e->td3_written;
    if (capacity) *capacity = e->td3_cfg.capacity;
    if (batch_size) *batch_size = e->td3_cfg.batch_size;
    return ADC_OK;
}
int off_ring_fetch(adc_engine *e, int member, int64_t slot, int64_t count, float *x, float *a, float *r, uint8_t *done, float *x2)
{
    if (slot < 0 || count < 1 || slot > td3_size(e) - count) return fail(ADC_EINVAL, "the slot range is not inside [0, size)");
    ENGINE_GUARD(e);
    const size_t s = (size_t)slot, n = (size_t)count, D = (size_t)e->td3_shape.D, A = (size_t)e->td3_shape.A;
    const Td3Ring &g = off_ring(e, member);
    if (x) HIP_TRY(hipMemcpyAsync(x, g.x + s * D, n * D * 4, hipMemcpyDeviceToHost, e->stream));
    if (a) HIP_TRY(hipMemcpyAsync(a, g.a + s * A, n * A * 4, hipMemcpyDeviceToHost, e->stream));
    if (r) HIP_TRY(hipMemcpyAsync(r, g.r + s, n * 4, hipMemcpyDeviceToHost, e->stream));
    if (done) HIP_TRY(hipMemcpyAsync(done, g.done + s, n, hipMemcpyDeviceToHost, e->stream));
    if (x2) HIP_TRY(hipMemcpyAsync(x2, g.x2 + s * D, n * D * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}
int off_ring_load(adc_engine *e, int member, int64_t slot, int64_t count, const float *x, const float *a, const float *r, const uint8_t *done, const float *x2,
                  int64_t written)
{
    if (!x || !a || !r || !done || !x2) return fail(ADC_EINVAL, "x, a, r, done or x2 is NULL");
    if (slot < 0 || count < 1 || slot > (int64_t)e->td3_cfg.capacity - count) return fail(ADC_EINVAL, "the slot range is not inside [0, capacity)");
    if (written < slot + count) return fail(ADC_EINVAL, "written: at least slot + count");
    ENGINE_GUARD(e);
    const size_t s = (size_t)slot, n = (size_t)count, D = (size_t)e->td3_shape.D, A = (size_t)e->td3_shape.A;
    const Td3Ring &g = off_ring(e, member);
    HIP_TRY(hipMemcpyAsync(g.x + s * D, x, n * D * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(g.a + s * A, a, n * A * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(g.r + s, r, n * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(g.done + s, done, n, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(g.x2 + s * D, x2, n * D * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->td3_written = written;               // (a population's rings move together: one count for all)
    if (e->per_live) {
        if (int rc = per_loaded_run(e, (int)off_m(member), slot, count)) return rc;
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    return ADC_OK;
}
// the slots update number `update` reads under `key` at the ring's current size; `empty`: the front end's words for an empty ring
int off_batch_indices(adc_engine *e, uint64_t key, int64_t update, int32_t *idx_b, const char *empty)
{
    if (!idx_b) return fail(ADC_EINVAL, "idx_b is NULL");
    if (update < 0 || update >= 0xFFFFFFFFll) return fail(ADC_EINVAL, "update: 0 to 2^32 - 2");
    if (td3_size(e) == 0) return fail(ADC_ESTATE, empty);
    if (e->per_live) return fail(ADC_ESTATE, "prioritised replay is alive on this engine: the batch is adc_engine_replay_prio_batch's, not the uniform law's");
    ENGINE_GUARD(e);
    const int B = e->td3_cfg.batch_size;
    hipLaunchKernelGGL(k_td3_indices, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, e->stream, key, (uint32_t)update, (uint32_t)td3_size(e), B, e->td3_idx);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(idx_b, e->td3_idx, (size_t)B * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

// ---- the state vectors ---------------------------------------------------------------------------------------------------------
int off_param_counts(const adc_engine *e, int64_t *actor_p, int64_t *critics_2qc)
{
    if (actor_p) *actor_p = e->td3_P;
    if (critics_2qc) *critics_2qc = 2 * (int64_t)e->td3_Qc;
    return ADC_OK;
}
// the copies of a member's flat vectors and moments to the host, those asked for; the caller waits for the stream
int off_state_get(adc_engine *e, int member, float *const flat[4], float *const mom[4])
{
    const size_t mi = off_m(member);
    for (int w = 0; w < 4; ++w) {
        const size_t fq = tp_count(e, w), mq = tp_count(e, w < 2 ? kTd3Theta : kTd3Psi);
        if (flat[w]) HIP_TRY(hipMemcpyAsync(flat[w], e->td3_flat[w] + mi * fq, fq * 4, hipMemcpyDeviceToHost, e->stream));
        if (mom[w]) HIP_TRY(hipMemcpyAsync(mom[w], e->td3_mom[w] + mi * mq, mq * 4, hipMemcpyDeviceToHost, e->stream));
    }
    return ADC_OK;
}
// a member's moments and flat vectors from the host, its stores after them, the wait, the update counter, the critics' flags.  A
// null flat[w] is skipped: SAC's target actor, which does not exist (its moments come all the same; TD3's front ends refuse a
// null vector before they call)
int off_state_set(adc_engine *e, int member, const float *const flat[4], const float *const mom[4], int64_t updates)
{
    const size_t mi = off_m(member);
    for (int w = 0; w < 4; ++w) {
        const size_t fq = tp_count(e, w), mq = tp_count(e, w < 2 ? kTd3Theta : kTd3Psi);
        HIP_TRY(hipMemcpyAsync(e->td3_mom[w] + mi * mq, mom[w], mq * 4, hipMemcpyHostToDevice, e->stream));
        if (!flat[w]) continue;
        HIP_TRY(hipMemcpyAsync(e->td3_flat[w] + mi * fq, flat[w], fq * 4, hipMemcpyHostToDevice, e->stream));
        off_params_copy(e, w, member, 1, 0);        // (the policy layers, the critics and the targets follow the flat vectors)
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->td3_updates = updates;               // (a population's members move together: one counter for all)
    off_critics_mark(e, member);
    return ADC_OK;
}
// member src's vectors, moments and critic flags into member dst (with_ring: its ring and the replay priorities too); a vector
// the trainer does not have (SAC's target actor) is skipped
int off_pop_copy(adc_engine *e, int src, int dst, int with_ring)
{
    const size_t from = (size_t)src, to = (size_t)dst;
    for (int w = 0; w < 4; ++w) {
        const size_t fq = tp_count(e, w), mq = tp_count(e, w < 2 ? kTd3Theta : kTd3Psi);
        HIP_TRY(hipMemcpyAsync(e->td3_mom[w] + to * mq, e->td3_mom[w] + from * mq, mq * 4, hipMemcpyDeviceToDevice, e->stream));
        if (!e->td3_flat[w]) continue;
        HIP_TRY(hipMemcpyAsync(e->td3_flat[w] + to * fq, e->td3_flat[w] + from * fq, fq * 4, hipMemcpyDeviceToDevice, e->stream));
        tp_params_copy(e, w, dst, 1, 0);
    }
    HIP_TRY(hipGetLastError());
    if (with_ring) {
        const size_t C = (size_t)e->td3_cfg.capacity, D = (size_t)e->td3_shape.D, A = (size_t)e->td3_shape.A;
        const Td3Ring &s = e->tp_mem[from].ring, &d = e->tp_mem[to].ring;
        HIP_TRY(hipMemcpyAsync(d.x, s.x, C * D * 4, hipMemcpyDeviceToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(d.a, s.a, C * A * 4, hipMemcpyDeviceToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(d.r, s.r, C * 4, hipMemcpyDeviceToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(d.done, s.done, C, hipMemcpyDeviceToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(d.x2, s.x2, C * D * 4, hipMemcpyDeviceToDevice, e->stream));
        if (s.gn) HIP_TRY(hipMemcpyAsync(d.gn, s.gn, C * 4, hipMemcpyDeviceToDevice, e->stream));      // (n-step returns: the slots' discounts)
        if (e->per_live)
            if (int rc = per_copy_run(e, src, dst)) return rc;      // (the leaves, nodes and top travel with the ring)
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < kOffCriticFlags; ++i) e->tp_critic_set[to * kOffCriticFlags + i] = e->tp_critic_set[from * kOffCriticFlags + i];
    return ADC_OK;
}

// ---- allocation ----------------------------------------------------------------------------------------------------------------
// the buffers every front end has, for M members (the solo trainers: 1); ring: the members' rings one after the other
struct OffBufs {
    float *flat[4] = {}, *mom[4] = {}, *grad = nullptr, *ybuf = nullptr, *xin = nullptr, *acts = nullptr, *deltas = nullptr, *pieces = nullptr;
    int32_t *idx = nullptr;
    double *part = nullptr, *sums = nullptr, *gpart = nullptr;
    Td3Ring ring{};
    size_t P = 0, Qc = 0, part_stride = 0;
};
int off_alloc(adc_engine *e, std::vector<void *> &fresh, const adc::Td3Shape &sh, int B, size_t C, size_t M, bool target_actor, OffBufs &o)
{
    const size_t A = (size_t)sh.A, D = (size_t)sh.D, P = (size_t)adc::td3_params(sh.pol), Q2 = 2 * (size_t)adc::td3_params(sh.q), Qmax = std::max(P, Q2);
    const size_t na = (size_t)std::max(std::max(2 * adc::td3_hidden(sh.q), adc::td3_hidden(sh.pol)), 1);
    const size_t nd = (size_t)std::max(2 * adc::td3_outs(sh.q), adc::td3_outs(sh.pol));
    o.P = P; o.Qc = Q2 / 2; o.part_stride = (size_t)pg_chunks((long long)std::max((size_t)B, Qmax)) * 8u + 8u;
    int rc = ADC_OK;
    for (int w = 0; w < 4 && !rc; ++w) {
        if (w != kTd3ThetaT || target_actor) rc = mlp_alloc(e, fresh, &o.flat[w], M * ((w & 1) ? Q2 : P));
        if (!rc) rc = mlp_alloc(e, fresh, &o.mom[w], M * (w < 2 ? P : Q2));
    }
    if (rc || (rc = mlp_alloc(e, fresh, &o.grad, M * Qmax)) || (rc = mlp_alloc(e, fresh, &o.ybuf, M * (size_t)B)) ||
        (rc = mlp_alloc(e, fresh, &o.xin, M * (size_t)B * (D + A))) || (rc = mlp_alloc(e, fresh, &o.acts, M * (size_t)B * na)) ||
        (rc = mlp_alloc(e, fresh, &o.deltas, M * (size_t)B * nd)) || (rc = mlp_alloc(e, fresh, &o.pieces, M * (size_t)B * (size_t)adc::kTd3Pieces)) ||
        (rc = mlp_alloc(e, fresh, &o.idx, (size_t)B)) || (rc = mlp_alloc(e, fresh, &o.part, M * o.part_stride)) || (rc = mlp_alloc(e, fresh, &o.sums, M * 16u)) ||
        (rc = mlp_alloc(e, fresh, &o.gpart, M * (size_t)pg_chunks(B) * Qmax)) || (rc = mlp_alloc(e, fresh, &o.ring.x, M * C * D)) ||
        (rc = mlp_alloc(e, fresh, &o.ring.a, M * C * A)) || (rc = mlp_alloc(e, fresh, &o.ring.r, M * C)) || (rc = mlp_alloc(e, fresh, &o.ring.done, M * C)) ||
        (rc = mlp_alloc(e, fresh, &o.ring.x2, M * C * D)))
        return rc;
    return ADC_OK;
}
// the engine's fields of those buffers (after td3_drop); the ring is the front end's to place
void off_install(adc_engine *e, const OffBufs &o, const adc::Td3Shape &sh)
{
    e->td3_shape = sh;
    e->td3_P = (int)o.P; e->td3_Qc = (int)o.Qc;
    for (int w = 0; w < 4; ++w) { e->td3_flat[w] = o.flat[w]; e->td3_mom[w] = o.mom[w]; }
    e->td3_grad = o.grad; e->td3_ybuf = o.ybuf; e->td3_xin = o.xin; e->td3_acts = o.acts; e->td3_deltas = o.deltas; e->td3_pieces = o.pieces; e->td3_idx = o.idx;
    e->td3_part = o.part; e->td3_sums = o.sums; e->td3_gpart = o.gpart;
    e->td3_stored_t = e->ro_t;              // (days recorded before this call are not the trainer's)
}
// the solo trainers' stores, one allocation per layer: `count` networks, the first four the critics' shape, a fifth the policy's
int off_solo_nets(adc_engine *e, std::vector<void *> &fresh, const adc::Td3Shape &sh, MlpNet *nets, int count)
{
    for (int n = 0; n < count; ++n) {
        const adc::Td3Net &shape = n < 4 ? sh.q : sh.pol;
        nets[n].layers = shape.layers;
        for (int l = 0; l < shape.layers; ++l) {
            float *w = nullptr, *b = nullptr;
            const int n_in = adc::td3_n_in(shape, l), n_out = shape.n_out[l];
            int rc;
            if ((rc = mlp_alloc(e, fresh, &w, adc::mlp_weight_count(n_in, n_out))) || (rc = mlp_alloc(e, fresh, &b, (size_t)n_out))) return rc;
            nets[n].W[l] = w; nets[n].b[l] = b; nets[n].n_in[l] = n_in; nets[n].n_out[l] = n_out;
        }
    }
    return ADC_OK;
}
// a population member's block of stores: critic 1, critic 2, target critic 1, target critic 2 and (count = 5) the target actor,
// every piece on a 16-byte boundary
struct OffBlock {
    size_t offW[5][adc::kMlpMaxLayers] = {}, offb[5][adc::kMlpMaxLayers] = {}, stride = 0;
};
OffBlock off_block_layout(const adc::Td3Shape &sh, int count)
{
    OffBlock k;
    for (int n = 0; n < count; ++n) {
        const adc::Td3Net &shape = n < 4 ? sh.q : sh.pol;
        for (int l = 0; l < shape.layers; ++l) {
            k.offW[n][l] = k.stride; k.stride += adc::mlp_weight_count(adc::td3_n_in(shape, l), shape.n_out[l]);
            k.offb[n][l] = k.stride; k.stride += ((size_t)shape.n_out[l] + 3u) & ~(size_t)3u;
        }
    }
    return k;
}
// member m's networks in its block at `block`, its ring among the members' rings
void off_member_place(Td3Member &me, size_t m, const OffBlock &k, int count, float *block, const OffBufs &o, const adc::Td3Shape &sh, size_t C)
{
    float *base = block + m * k.stride;
    MlpNet *nets[5] = {&me.q[0], &me.q[1], &me.q_t[0], &me.q_t[1], &me.pol_t};
    for (int n = 0; n < count; ++n) {
        const adc::Td3Net &shape = n < 4 ? sh.q : sh.pol;
        nets[n]->layers = shape.layers;
        for (int l = 0; l < shape.layers; ++l) {
            nets[n]->W[l] = base + k.offW[n][l]; nets[n]->b[l] = base + k.offb[n][l];
            nets[n]->n_in[l] = adc::td3_n_in(shape, l); nets[n]->n_out[l] = shape.n_out[l];
        }
    }
    const size_t D = (size_t)sh.D, A = (size_t)sh.A;
    me.ring = Td3Ring{o.ring.x + m * C * D, o.ring.a + m * C * A, o.ring.r + m * C, o.ring.x2 + m * C * D, o.ring.done + m * C, nullptr};
}

// ---- an update's launches ------------------------------------------------------------------------------------------------------
adc::EsStep td3_step_of(const adc_td3_config &c, float lr, int64_t steps_taken)
{
    adc::EsStep step{};
    step.optimiser = c.optimiser == ADC_TD3_SGD ? adc::kEsSgd : adc::kEsAdam;
    step.lr = lr; step.beta1 = c.beta1; step.beta2 = c.beta2; step.eps = c.eps; step.l2 = 0.0f;
    step.c1 = adc::es_bias_correction(step.beta1, (uint32_t)(steps_taken + 1));
    step.c2 = adc::es_bias_correction(step.beta2, (uint32_t)(steps_taken + 1));
    return step;
}
// prioritised replay's side of a batch kernel's view (all null without adc_engine_replay_prio_init: the kernels are what they were)
template <class BatchView>
void td3_per_fill(const adc_engine *e, BatchView &p)
{
    if (!e->per_live) return;
    p.p_slot = e->per.slot; p.p_w = e->per.w; p.p_absd = e->per.absd;
}
int td3_csum_launch(adc_engine *e, const float *src, long long n, int stride, int cols, int mode, double *out)
{
    const long long chunks = pg_chunks(n), lanes = chunks * cols;
    hipLaunchKernelGGL(k_pg_chunk_sums, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, e->stream, src, n, stride, cols, mode, 0.0, e->td3_part);
    hipLaunchKernelGGL(k_pg_join, dim3(1), dim3(64), 0, e->stream, e->td3_part, chunks, cols, out);
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}
// the weight gradient's partials of one network over the batch: its first layer's X is the gathered rows
void td3_wgrad_launch(adc_engine *e, const adc::Td3Net &net, int ldx0, int na, int acts_off, int nd, int d_off, int flat0, int Q, int B)
{
    int flat = flat0, ao = acts_off, dof = d_off;
    for (int l = 0; l < net.layers; ++l) {
        const int n_in = adc::td3_n_in(net, l), n_out = net.n_out[l];
        PgTerm t{l == 0 ? e->td3_xin : e->td3_acts + ao, l == 0 ? (size_t)ldx0 : (size_t)na, n_in, n_out, dof, flat, 0};
        const unsigned tiles = (unsigned)(((n_in + 1 + kPgTile - 1) / kPgTile) * ((n_out + kPgTile - 1) / kPgTile));
        hipLaunchKernelGGL(k_pg_wgrad, dim3(tiles, (unsigned)pg_chunks(B)), dim3(kPgBlock), 0, e->stream, t, (long long)B, 1, 1, 0, e->td3_deltas, nd,
                           e->td3_gpart, Q);
        flat += (n_in + 1) * n_out;
        dof += n_out;
        if (l > 0) ao += n_in;
    }
}
// the gradient in td3_grad from the partials, its squared norm into sums[slot] when asked for, the clip's scale, the step
int td3_step_run(adc_engine *e, int which, float **mom, int Q, int B, bool norm_wanted, int slot, float lr, int64_t steps_taken)
{
    hipLaunchKernelGGL(k_pg_grad_join, dim3((unsigned)((Q + kPgBlock - 1) / kPgBlock)), dim3(kPgBlock), 0, e->stream, e->td3_gpart, (int)pg_chunks(B), Q,
                       (long long)B, e->td3_grad);
    HIP_TRY(hipGetLastError());
    const bool clip = e->td3_cfg.max_grad_norm > 0.0f;
    float scale = 1.0f;
    if (clip || norm_wanted)
        if (int rc = td3_csum_launch(e, e->td3_grad, Q, 1, 1, 2, e->td3_sums + slot)) return rc;
    if (clip) {
        double sq = 0.0;
        HIP_TRY(hipMemcpyAsync(&sq, e->td3_sums + slot, 8, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        scale = adc::pg_clip_scale(e->td3_cfg.max_grad_norm, std::sqrt(sq));
    }
    hipLaunchKernelGGL(k_pg_update, dim3((unsigned)((Q + kPgBlock - 1) / kPgBlock)), dim3(kPgBlock), 0, e->stream, e->td3_lay[which], e->td3_flat[which],
                       mom[0], mom[1], e->td3_grad, clip ? 1 : 0, scale, td3_step_of(e->td3_cfg, lr, steps_taken));
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}
// every member's chunked sum of `cols` columns (its rows from member * mstep on) into td3_sums[member * 16 + at ...]
int tp_csum_launch(adc_engine *e, const float *src, int n, size_t mstep, int stride, int cols, int mode, int at)
{
    const int chunks = (int)pg_chunks(n), lanes = chunks * cols, M = e->lrn_M;
    hipLaunchKernelGGL(k_pg_pop_chunk_sums, dim3((unsigned)((lanes + 255) / 256), (unsigned)M), dim3(256), 0, e->stream, src, n, 0, 0, mstep, stride, cols, mode,
                       (const PgMember *)nullptr, e->td3_part, e->tp_part_stride);
    hipLaunchKernelGGL(k_pg_pop_join, dim3((unsigned)M), dim3(64), 0, e->stream, e->td3_part, e->tp_part_stride, chunks, cols, e->td3_sums + at, 16);
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}
// the weight gradient's partials of one network of every member over its batch
void tp_wgrad_launch(adc_engine *e, const adc::Td3Net &net, int ldx0, int na, int acts_off, int nd, int d_off, int flat0, int Q, int B)
{
    int flat = flat0, ao = acts_off, dof = d_off;
    for (int l = 0; l < net.layers; ++l) {
        const int n_in = adc::td3_n_in(net, l), n_out = net.n_out[l];
        PgTerm t{l == 0 ? e->td3_xin : e->td3_acts + ao, l == 0 ? (size_t)ldx0 : (size_t)na, n_in, n_out, dof, flat, 0};
        const unsigned tiles = (unsigned)(((n_in + 1 + kPgTile - 1) / kPgTile) * ((n_out + kPgTile - 1) / kPgTile));
        hipLaunchKernelGGL(k_pg_pop_wgrad, dim3(tiles, (unsigned)pg_chunks(B), (unsigned)e->lrn_M), dim3(kPgBlock), 0, e->stream, t, (long long)B, 1, 1, 0, 0,
                           e->td3_deltas, nd, e->td3_gpart, Q);
        flat += (n_in + 1) * n_out;
        dof += n_out;
        if (l > 0) ao += n_in;
    }
}
// every member's gradient from the partials, its squared norm into sums[slot] when asked for, the clip's scale, the step
int tp_step_run(adc_engine *e, int which, float **mom, int Q, int B, bool norm_wanted, int slot, int row, bool any_clip)
{
    const int M = e->lrn_M;
    hipLaunchKernelGGL(k_pg_pop_grad_join, dim3(pg_blocks(Q), (unsigned)M), dim3(kPgBlock), 0, e->stream, e->td3_gpart, (int)pg_chunks(B), Q, (long long)B,
                       e->td3_grad);
    HIP_TRY(hipGetLastError());
    if (any_clip || norm_wanted)
        if (int rc = tp_csum_launch(e, e->td3_grad, Q, (size_t)Q, 1, 1, 2, slot)) return rc;
    Td3PopStep *drow = e->tp_dsteps + (size_t)row * (size_t)M;
    if (any_clip) {
        // all members' squared norms in one copy, each scale finished on the host as the solo path's is, the row up in one copy
        HIP_TRY(hipMemcpyAsync(e->tp_host_sums.data(), e->td3_sums, e->tp_host_sums.size() * 8, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        Td3PopStep *hrow = e->tp_steps.data() + (size_t)row * (size_t)M;
        for (int m = 0; m < M; ++m) {
            const float mgn = e->tp_cfg[(size_t)m].max_grad_norm;
            hrow[m].clip = mgn > 0.0f;
            hrow[m].scale = hrow[m].clip ? adc::pg_clip_scale(mgn, std::sqrt(e->tp_host_sums[(size_t)m * 16 + (size_t)slot])) : 1.0f;
        }
        HIP_TRY(hipMemcpyAsync(drow, hrow, (size_t)M * sizeof(Td3PopStep), hipMemcpyHostToDevice, e->stream));
    }
    hipLaunchKernelGGL(k_td3_pop_step, dim3(pg_blocks(Q), (unsigned)M), dim3(kPgBlock), 0, e->stream, e->td3_lay[which], e->tp_stride[which], e->td3_flat[which],
                       mom[0], mom[1], e->td3_grad, drow);
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}

// ---- a call's updates ----------------------------------------------------------------------------------------------------------
// what every *_update refuses; `unset` and `empty` are the front end's words.  `bound`: the counter's end, 0xFFFFFFFF for TD3 and
// its populations, 0x7FFFFFFF for SAC and its populations - as each front end had it; the state_set bounds are 0x7FFFFFFF in all
int off_update_check(const adc_engine *e, int32_t updates, bool pop, const char *unset, const char *empty, int64_t bound)
{
    if (updates < 1 || updates > 65536) return fail(ADC_EINVAL, "updates: 1 to 65536");
    if (!off_critics_set(e, pop)) return fail(ADC_ESTATE, unset);
    if (td3_size(e) == 0) return fail(ADC_ESTATE, empty);
    if (e->td3_updates + updates >= bound) return fail(ADC_ESTATE, "the update counter is exhausted");
    return ADC_OK;
}
// updates of a call whose step constants go up in one copy (a longer call waits for the stream once per so many updates)
constexpr int kTd3PopBlock = 64;
// a population's `updates` updates, `rows` rows of the step table each (TD3: critic, actor; SAC: critic, actor, temperature):
// fill(nb) writes the host's rows of the next nb updates, one(u, i) launches update u of the call, the i-th of its block
template <class Fill, class One>
int off_pop_updates(adc_engine *e, int32_t updates, size_t rows, Fill fill, One one)
{
    const size_t M = (size_t)e->lrn_M;
    HIP_TRY(hipMemsetAsync(e->td3_sums, 0, M * 16 * sizeof(double), e->stream));
    for (int u0 = 0; u0 < updates; u0 += kTd3PopBlock) {
        const int nb = std::min(kTd3PopBlock, updates - u0);
        // the block's step constants (the Adam bias corrections of every step to come) in one copy; the host's table is free to
        // write: the call before this one, and the block before this one, ended with a wait
        if (u0 > 0) HIP_TRY(hipStreamSynchronize(e->stream));
        fill(nb);
        HIP_TRY(hipMemcpyAsync(e->tp_dsteps, e->tp_steps.data(), (size_t)nb * rows * M * sizeof(Td3PopStep), hipMemcpyHostToDevice, e->stream));
        for (int i = 0; i < nb; ++i)
            if (int rc = one(u0 + i, i)) return rc;
    }
    return ADC_OK;
}
// the fields adc_td3_stats and adc_sac_stats share, from one learner's sums
template <class Stats>
void off_stats_fill(const adc_engine *e, const double *sums, Stats *stats)
{
    const double n = (double)e->td3_cfg.batch_size;
    const double l1 = sums[adc::kTd3Loss1] / n, l2 = sums[adc::kTd3Loss2] / n;
    stats->updates = e->td3_updates; stats->buffer_size = td3_size(e); stats->samples = e->td3_cfg.batch_size;
    stats->critic_loss = l1 + l2;
    stats->q1_mean = sums[adc::kTd3Q1] / n; stats->q2_mean = sums[adc::kTd3Q2] / n; stats->y_mean = sums[adc::kTd3Y] / n;
}
}  // namespace
