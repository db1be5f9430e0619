// pg_shuffle_api.inc - the extern "C" entry points of the PPO / A2C learners' shuffled sample-level minibatches and target-KL early
// stop (include/adcraft_engine.h; the kernels are parts/kernel_pg_shuffle.inc, the law csrc/adc_pg_shuffle.h), and what
// parts/pg_api.inc calls of the add-on: the start of an update, the bookkeeping of an evaluated minibatch, the update loops under
// it.  The order of an epoch is never kept on the host: a member's key and the tick its order was drawn with are one small table,
// uploaded once per epoch whatever M is.  A minibatch costs what it costs without the add-on - its statistics come to the host
// before the step, as the norm clip's scale needs them anyway - so the early stop adds no round trip.
// (part of the single translation unit adc_engine.hip)
namespace {
constexpr const char *kShNotReady =
    "adc_engine_pg_shuffle_init has not been called (or the trainer, the policy, the learners or the record were re-initialised since)";

int sh_minibatches(const adc_engine *e) { return (int)(((long long)e->sh_ns + e->sh_mb - 1) / e->sh_mb); }

// the advantages have been computed: a new update begins, no member has stopped, an order has yet to be drawn
void sh_update_begin(adc_engine *e)
{
    e->sh_epoch_ready = false;
    e->sh_stats.assign(e->sh_stats.size(), adc_pg_shuffle_stats{});
    std::fill(e->sh_evaluated.begin(), e->sh_evaluated.end(), (uint8_t)0);
}

// member m's gathered minibatch of S samples has reached the host with approx_kl: true when its step is to be taken.  A member
// that had stopped before is not counted; one that stops now is (the stopping minibatch belongs to the statistics)
bool sh_minibatch_evaluated(adc_engine *e, int m, double approx_kl, long long S)
{
    adc_pg_shuffle_stats &st = e->sh_stats[(size_t)m];
    if (st.stopped) { e->sh_evaluated[(size_t)m] = 0; return false; }
    e->sh_evaluated[(size_t)m] = 1;
    e->sh_last_count[(size_t)m] = S;
    st.minibatches_evaluated += 1;
    if (adc::pg_shuffle_stop(approx_kl, e->sh_cfg[(size_t)m].target_kl)) { st.stopped = 1; return false; }
    st.steps_taken += 1;
    return true;
}

bool sh_all_stopped(const adc_engine *e)
{
    for (const adc_pg_shuffle_stats &st : e->sh_stats)
        if (!st.stopped) return false;
    return true;
}

// the order of a new epoch for every member: its tick is the member's step count now
int sh_epoch_run(adc_engine *e)
{
    const int M = pg_members(e), n = pg_member_envs(e);
    const uint32_t n_s = (uint32_t)e->ro_t * (uint32_t)n;
    HIP_TRY(hipStreamSynchronize(e->stream));       // (the last epoch's upload of the host's table may still be in flight)
    for (int m = 0; m < M; ++m) {
        e->sh_mem[(size_t)m].tick = (uint32_t)((uint64_t)e->pgp_steps[(size_t)m] & 0xFFFFFFFFull);
        if (!e->sh_stats[(size_t)m].stopped) e->sh_stats[(size_t)m].epochs_begun += 1;
    }
    HIP_TRY(hipMemcpyAsync(e->sh_dmem, e->sh_mem.data(), e->sh_mem.size() * sizeof(PgShuffleMember), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_pg_shuffle_rows, dim3((n_s + 255u) / 256u, (unsigned)M), dim3(256), 0, e->stream, e->sh_dmem, n_s, adc::pg_shuffle_half_bits(n_s),
                       (uint32_t)n, (uint32_t)e->v.N, e->sh_order, e->sh_rows);
    HIP_TRY(hipGetLastError());
    e->sh_ns = n_s;
    e->sh_epoch_ready = true;
    return ADC_OK;
}

PgGather sh_gather(const adc_engine *e, int j)
{
    const long long at = (long long)j * e->sh_mb, left = (long long)e->sh_ns - at;
    return PgGather{e->sh_rows + at, (size_t)e->sh_ns, left < e->sh_mb ? left : (long long)e->sh_mb};
}

// adc_engine_pg_update / _pg_pop_update under the add-on, after the advantages: per epoch a new order and its ceil(n_s / mb)
// minibatches, every member until it stops; the statistics of the last epoch a member began
int sh_update_run(adc_engine *e, int epochs, adc_pg_stats *stats_m)
{
    const int M = pg_members(e);
    std::vector<adc::PgStatsOut> o((size_t)M), acc((size_t)M), mean((size_t)M);
    std::vector<int> cnt((size_t)M, 0);
    std::vector<uint8_t> live((size_t)M, 1);
    KlEpoch kl;
    int rc;
    for (int ep = 0; ep < epochs && !sh_all_stopped(e); ++ep) {
        if ((rc = sh_epoch_run(e))) return rc;
        for (int m = 0; m < M; ++m) {
            live[(size_t)m] = !e->sh_stats[(size_t)m].stopped;
            if (live[(size_t)m]) { acc[(size_t)m] = adc::PgStatsOut{}; cnt[(size_t)m] = 0; }
        }
        kl.begin(e, live.data());
        const int count = sh_minibatches(e);
        for (int j = 0; j < count && !sh_all_stopped(e); ++j) {
            const PgGather g = sh_gather(e, j);
            if ((rc = pg_gathered_run(e, o.data(), &g))) return rc;
            kl.add(e, e->sh_evaluated.data());
            for (int m = 0; m < M; ++m)
                if (e->sh_evaluated[(size_t)m]) { pg_stats_add(acc[(size_t)m], o[(size_t)m]); cnt[(size_t)m] += 1; }
        }
        for (int m = 0; m < M; ++m)
            if (live[(size_t)m]) mean[(size_t)m] = pg_stats_mean(acc[(size_t)m], cnt[(size_t)m]);
    }
    if (e->kl_live && (rc = kl_update_end(e, kl))) return rc;
    if (stats_m)
        for (int m = 0; m < M; ++m) pg_stats_fill(stats_m + m, mean[(size_t)m], e->pgp_steps[(size_t)m], e->sh_last_count[(size_t)m]);
    return ADC_OK;
}

// one of the trainer's arrays grown: the old one leaves the trainer's allocations
template <typename T>
void sh_replace(adc_engine *e, T *&slot, T *fresh)
{
    auto it = std::find(e->pg_allocs.begin(), e->pg_allocs.end(), (void *)slot);
    if (it != e->pg_allocs.end()) e->pg_allocs.erase(it);
    (void)hipFree(slot);
    slot = fresh;
}
}  // namespace

ADC_EXPORT int adc_engine_pg_shuffle_init(adc_engine *e, const adc_pg_shuffle_config *cfgs, int32_t count)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (e->have_td3 || e->have_td3_pop)
        return fail(ADC_ESTATE, "an off-policy (TD3) trainer is alive on this engine: its batches are drawn per update already (shuffled minibatches belong to PPO / A2C)");
    if (!e->have_pg && !e->have_pg_pop)
        return fail(ADC_ESTATE, "shuffled minibatches are an add-on to a PPO / A2C trainer: adc_engine_pg_init or adc_engine_pg_pop_init first");
    if (e->have_im) return fail(ADC_ESTATE, "imitation is alive on this trainer (adc_engine_im_init): its updates run over contiguous env minibatches");
    const int M = pg_members(e), n = pg_member_envs(e);
    if (!cfgs) return fail(ADC_EINVAL, "adc_pg_shuffle_config array is NULL");
    if (count != 1 && count != M) return fail(ADC_EINVAL, "count: 1 (one configuration shared by all members) or the number of members");
    for (int i = 0; i < count; ++i) {
        const char *why = nullptr;
        if (adc_pg_shuffle_config_check(cfgs + i, &why) != ADC_OK) return fail(ADC_EINVAL, why);
        if (cfgs[i].minibatch_samples != cfgs[0].minibatch_samples)
            return fail(ADC_EINVAL, "minibatch_samples must be equal in all members: their minibatches run in the same launches");
    }
    const size_t cap = (size_t)e->ro_T * (size_t)n, mb = (size_t)cfgs[0].minibatch_samples;
    if (mb > cap) return fail(ADC_EINVAL, "minibatch_samples: at most horizon x envs of a member");
    if ((size_t)e->ro_T * (size_t)e->v.N > 0x7FFFFFFFull) return fail(ADC_EINVAL, "horizon x num_envs: at most 2^31 - 1 recorded rows under shuffled minibatches");
    const size_t slots = std::max(e->pg_slots, mb);
    if (pg_chunks((long long)slots) > 65535) return fail(ADC_EINVAL, "minibatch_samples: at most 65535 x 1024 samples in a minibatch");
    ENGINE_GUARD(e);
    const adc::PgShape &sh = e->pg_shape;
    const size_t Ms = (size_t)M, Q = (size_t)pg_Q(e);
    // (everything new is allocated before anything old goes: a refused allocation leaves the engine as it was)
    std::vector<void *> fresh;
    float *acts = nullptr, *deltas = nullptr, *pieces = nullptr, *klp = nullptr;
    double *gpart = nullptr;
    uint32_t *order = nullptr, *rows = nullptr;
    PgShuffleMember *dmem = nullptr;
    int rc = ADC_OK;
    const bool grow = slots > e->pg_slots, own = !e->sh_rows;
    if ((grow && ((rc = mlp_alloc(e, fresh, &acts, Ms * slots * (size_t)adc::pg_acts_floats(sh))) ||
                  (rc = mlp_alloc(e, fresh, &deltas, Ms * slots * (size_t)adc::pg_deltas_floats(sh))) ||
                  (rc = mlp_alloc(e, fresh, &pieces, Ms * slots * (size_t)adc::kPgPieces)) ||
                  (rc = mlp_alloc(e, fresh, &gpart, Ms * (size_t)pg_chunks((long long)slots) * Q)) ||
                  (e->kl_pieces && (rc = mlp_alloc(e, fresh, &klp, Ms * slots * (size_t)adc::kPgKlPieces))))) ||
        (own && ((rc = mlp_alloc(e, fresh, &order, Ms * cap)) || (rc = mlp_alloc(e, fresh, &rows, Ms * cap)) || (rc = mlp_alloc(e, fresh, &dmem, Ms))))) {
        mlp_free(e, fresh);
        return rc;
    }
    if (const hipError_t err = hipStreamSynchronize(e->stream); err != hipSuccess) {       // (nothing old has gone yet)
        mlp_free(e, fresh);
        return fail(ADC_EHIP, std::string("hipStreamSynchronize(e->stream): ") + hipGetErrorString(err));
    }
    if (grow) {
        sh_replace(e, e->pg_acts, acts); sh_replace(e, e->pg_deltas, deltas); sh_replace(e, e->pg_pieces, pieces); sh_replace(e, e->pg_gpart, gpart);
        if (e->kl_pieces) sh_replace(e, e->kl_pieces, klp);
        e->pg_slots = slots;
    }
    if (own) { e->sh_order = order; e->sh_rows = rows; e->sh_dmem = dmem; }
    e->pg_allocs.insert(e->pg_allocs.end(), fresh.begin(), fresh.end());
    e->sh_cfg.assign(Ms, cfgs[0]);
    if (count > 1) e->sh_cfg.assign(cfgs, cfgs + M);
    e->sh_mem.assign(Ms, PgShuffleMember{});
    for (size_t m = 0; m < Ms; ++m) e->sh_mem[m].key = adc::pg_shuffle_key(e->sh_cfg[m].seed ? e->sh_cfg[m].seed : e->cfg.seed);
    e->sh_stats.assign(Ms, adc_pg_shuffle_stats{});
    e->sh_evaluated.assign(Ms, 0);
    e->sh_last_count.assign(Ms, 0);
    e->sh_mb = (int)mb;
    e->sh_ns = 0;
    e->sh_live = true;
    e->sh_epoch_ready = false;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_shuffle_epoch(adc_engine *e)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->sh_live) return fail(ADC_ESTATE, kShNotReady);
    int rc;
    if ((rc = pg_state_check(e, e->have_pg_pop)) || (rc = pg_record_check(e))) return rc;
    if (!e->pg_adv_ready)
        return fail(ADC_ESTATE, "adc_engine_pg_advantages / _pg_pop_advantages has not been called since the last recorded day (an update begins with it)");
    ENGINE_GUARD(e);
    return sh_epoch_run(e);
}

ADC_EXPORT int adc_engine_pg_shuffle_minibatch(adc_engine *e, int32_t index, adc_pg_stats *stats_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->sh_live) return fail(ADC_ESTATE, kShNotReady);
    int rc;
    if ((rc = pg_state_check(e, e->have_pg_pop)) || (rc = pg_record_check(e))) return rc;
    if (!e->pg_adv_ready)
        return fail(ADC_ESTATE, "adc_engine_pg_advantages / _pg_pop_advantages has not been called since the last recorded day");
    if (!e->sh_epoch_ready) return fail(ADC_ESTATE, "adc_engine_pg_shuffle_epoch has not been called since the advantages: no order has been drawn");
    if (index < 0 || index >= sh_minibatches(e)) return fail(ADC_EINVAL, "no such minibatch: 0 to ceil(samples of a member / minibatch_samples) - 1");
    ENGINE_GUARD(e);
    const int M = pg_members(e);
    std::vector<adc::PgStatsOut> o((size_t)M);
    const PgGather g = sh_gather(e, index);
    if ((rc = pg_gathered_run(e, o.data(), &g))) return rc;
    if (stats_m)
        for (int m = 0; m < M; ++m) pg_stats_fill(stats_m + m, o[(size_t)m], e->pgp_steps[(size_t)m], g.S);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_shuffle_order_fetch(adc_engine *e, uint32_t *order, uint32_t *rows)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->sh_live) return fail(ADC_ESTATE, kShNotReady);
    // (the order is [members][n_s] of the days recorded when it was drawn: once the record has moved it is no longer to be had)
    if (!e->pg_adv_ready)
        return fail(ADC_ESTATE, "the record or the trainer's configuration has changed since the advantages: the order drawn under them is gone");
    if (!e->sh_epoch_ready) return fail(ADC_ESTATE, "adc_engine_pg_shuffle_epoch has not been called since the advantages: no order has been drawn");
    ENGINE_GUARD(e);
    const size_t bytes = (size_t)pg_members(e) * (size_t)e->sh_ns * 4;
    if (order) HIP_TRY(hipMemcpyAsync(order, e->sh_order, bytes, hipMemcpyDeviceToHost, e->stream));
    if (rows) HIP_TRY(hipMemcpyAsync(rows, e->sh_rows, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_pg_shuffle_stats(adc_engine *e, adc_pg_shuffle_stats *stats_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->sh_live) return fail(ADC_ESTATE, kShNotReady);
    if (!stats_m) return fail(ADC_EINVAL, "stats_m is NULL");
    std::copy(e->sh_stats.begin(), e->sh_stats.end(), stats_m);
    return ADC_OK;
}
