// per_api.inc - the extern "C" entry points of prioritised replay (include/adcraft_engine.h; the kernels are parts/kernel_per.inc,
// the law csrc/adc_per.h), and what the TD3 / SAC trainers' stores, buffer loads, updates and member copies call of it (declared in
// td3_api.inc).  The add-on lives in the off-policy trainer's fields: its arrays are among td3_allocs and go with the trainer; a
// solo learner is member 0 of a population of one.  Everything here runs on the engine's own stream behind ENGINE_GUARD.
// (part of the single translation unit adc_engine.hip)
namespace {
int per_ready(const adc_engine *e)
{
    if (!e->per_live) return fail(ADC_ESTATE, "adc_engine_replay_prio_init has not been called (or its trainer was re-initialised since)");
    return ADC_OK;
}
inline bool per_pop(const adc_engine *e) { return e->have_td3_pop || e->have_sac_pop; }
inline int per_members(const adc_engine *e) { return per_pop(e) ? e->lrn_M : 1; }
int per_member_check(const adc_engine *e, int32_t member)
{
    if (member < 0 || member >= per_members(e)) return fail(ADC_EINVAL, "no such member");
    return ADC_OK;
}
inline adc::PerLaw per_law(const adc_engine *e) { return adc::PerLaw{e->per_cfg.alpha, e->per_cfg.beta, e->per_cfg.eps, e->per_cfg.cap}; }
// the nodes above the slots [lo, lo + n) of the members of `v` (M of them), level by level
void per_rebuild_range(adc_engine *e, const PerView &v, int M, long long lo, long long n)
{
    for (int l = 1; l <= v.levels; ++l) {
        const long long first = lo >> (6 * l), items = ((lo + n - 1) >> (6 * l)) - first + 1;
        hipLaunchKernelGGL(k_per_rebuild, dim3((unsigned)((items + 3) / 4), (unsigned)M), dim3(256), 0, e->stream, v, l, 0, first, items);
    }
}
// leaf = top over the slots [lo, lo + n) of the members of `v`, and the nodes above them
void per_fill_range(adc_engine *e, const PerView &v, int M, long long lo, long long n)
{
    hipLaunchKernelGGL(k_per_fill, dim3((unsigned)((n + 255) / 256), (unsigned)M), dim3(256), 0, e->stream, v, lo, n);
    per_rebuild_range(e, v, M, lo, n);
}
// every member's slots and weights of update `update` into the batch buffers
int per_sample_run(adc_engine *e, uint32_t update)
{
    const int M = per_members(e), B = e->per.B;
    hipLaunchKernelGGL(k_per_sample, dim3((unsigned)B, (unsigned)M), dim3(64), 0, e->stream, e->per, e->td3_key, per_pop(e) ? e->tp_dmem : nullptr, update,
                       (uint32_t)td3_size(e));
    hipLaunchKernelGGL(k_per_weights, dim3(1, (unsigned)M), dim3(256), 0, e->stream, e->per, e->per_cfg.beta);
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}
// after the critics' pass: the sampled slots' new leaves, top, and the nodes on their paths
int per_leaves_run(adc_engine *e)
{
    const int M = per_members(e), B = e->per.B;
    hipLaunchKernelGGL(k_per_priorities, dim3(1, (unsigned)M), dim3(256), 0, e->stream, e->per, per_law(e));
    hipLaunchKernelGGL(k_per_leaves, dim3((unsigned)((B + 255) / 256), (unsigned)M), dim3(256), 0, e->stream, e->per);
    for (int l = 1; l <= e->per.levels; ++l)
        hipLaunchKernelGGL(k_per_rebuild, dim3((unsigned)((B + 3) / 4), (unsigned)M), dim3(256), 0, e->stream, e->per, l, 1, 0ll, (long long)B);
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}
// after a store of `count` transitions per member behind `written_before`: their slots get top
int per_store_run(adc_engine *e, int64_t written_before, int64_t count)
{
    const int M = per_members(e);
    const long long C = e->per.n[0];
    if (count >= C) per_fill_range(e, e->per, M, 0, C);
    else {
        const long long start = written_before % C, n1 = std::min<long long>(count, C - start);
        per_fill_range(e, e->per, M, start, n1);
        if (count > n1) per_fill_range(e, e->per, M, 0, count - n1);
    }
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}
// after a buffer load of member's slots [slot, slot + count) (the ring's size may have moved, for all members): they get top, and
// so does a stored slot that has no leaf yet; a slot past the size gets 0; all nodes are rebuilt
int per_loaded_run(adc_engine *e, int member, int64_t slot, int64_t count)
{
    const int M = per_members(e);
    const long long C = e->per.n[0];
    hipLaunchKernelGGL(k_per_fill, dim3((unsigned)((count + 255) / 256), 1u), dim3(256), 0, e->stream, per_member(e->per, (size_t)member), (long long)slot,
                       (long long)count);
    hipLaunchKernelGGL(k_per_resize, dim3((unsigned)((C + 255) / 256), (unsigned)M), dim3(256), 0, e->stream, e->per, (long long)td3_size(e));
    per_rebuild_range(e, e->per, M, 0, C);
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}
// member src's leaves, nodes and top into member dst's (a member copy that carries the ring)
int per_copy_run(adc_engine *e, int src, int dst)
{
    const PerView s = per_member(e->per, (size_t)src), d = per_member(e->per, (size_t)dst);
    HIP_TRY(hipMemcpyAsync(d.leaf, s.leaf, e->per.stride[0] * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    for (int l = 1; l <= e->per.levels; ++l)
        HIP_TRY(hipMemcpyAsync(d.node[l], s.node[l], e->per.stride[l] * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(d.top, s.top, sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    return ADC_OK;
}
// the first `npairs` pairs of the scheduler's device table: every donor's tree into its destination's, in one launch
void per_pairs_launch(adc_engine *e, int npairs)
{
    const unsigned blocks = (unsigned)std::min<size_t>((e->per.stride[0] + 255) / 256, 256);
    hipLaunchKernelGGL(k_per_copy_pairs, dim3(blocks, (unsigned)npairs), dim3(256), 0, e->stream, e->per, e->pbt_dpairs);
}
}  // namespace

ADC_EXPORT int adc_engine_replay_prio_init(adc_engine *e, const adc_replay_prio_config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const char *why = nullptr;
    if (adc_replay_prio_config_check(cfg, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    if (!e->have_td3 && !e->have_sac && !e->have_td3_pop && !e->have_sac_pop)
        return fail(ADC_ESTATE, "prioritised replay needs a live TD3 or SAC trainer (adc_engine_td3_init / _sac_init / _td3_pop_init / _sac_pop_init)");
    ENGINE_GUARD(e);
    const size_t M = (size_t)per_members(e), B = (size_t)e->td3_cfg.batch_size;
    const adc::PerShape sh = adc::per_shape_of((int64_t)e->td3_cfg.capacity);
    e->per_live = false;
    if (!e->per.leaf) {
        // (the arrays join the trainer's allocations: what a failure leaves behind goes with it)
        PerView v{};
        v.levels = sh.levels; v.B = (int)B;
        int rc = ADC_OK;
        for (int l = 0; l <= sh.levels; ++l) {
            v.n[l] = sh.n[l];
            v.stride[l] = (size_t)((sh.n[l] + adc::kPerRadix - 1) / adc::kPerRadix) * adc::kPerRadix;
            if (l >= 1 && (rc = mlp_alloc(e, e->td3_allocs, &v.node[l], M * v.stride[l]))) return rc;
        }
        if ((rc = mlp_alloc(e, e->td3_allocs, &v.leaf, M * v.stride[0])) || (rc = mlp_alloc(e, e->td3_allocs, &v.top, M)) ||
            (rc = mlp_alloc(e, e->td3_allocs, &v.slot, M * B)) || (rc = mlp_alloc(e, e->td3_allocs, &v.leaf_b, M * B)) ||
            (rc = mlp_alloc(e, e->td3_allocs, &v.w, M * B)) || (rc = mlp_alloc(e, e->td3_allocs, &v.absd, 2 * M * B)) ||
            (rc = mlp_alloc(e, e->td3_allocs, &v.pab, M * B)))
            return rc;
        e->per = v;
    } else {
        // a second init starts over (the trainer, and so the shapes, are the same)
        HIP_TRY(hipMemsetAsync(e->per.leaf, 0, M * e->per.stride[0] * sizeof(float), e->stream));
    }
    const std::vector<float> ones(M, 1.0f);
    HIP_TRY(hipMemcpyAsync(e->per.top, ones.data(), M * sizeof(float), hipMemcpyHostToDevice, e->stream));
    e->per_cfg = *cfg;
    // a ring that already holds transitions: its slots get leaf 1
    const long long C = e->per.n[0];
    hipLaunchKernelGGL(k_per_resize, dim3((unsigned)((C + 255) / 256), (unsigned)M), dim3(256), 0, e->stream, e->per, (long long)td3_size(e));
    per_rebuild_range(e, e->per, (int)M, 0, C);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));       // (`ones` is read until here)
    e->per_live = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_replay_prio_set_beta(adc_engine *e, float beta)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = per_ready(e)) return rc;
    if (!(beta >= 0.0f && beta <= 1.0f)) return fail(ADC_EINVAL, "beta must be in [0, 1]");
    e->per_cfg.beta = beta;             // (a launch carries the value in force when it is enqueued)
    return ADC_OK;
}

ADC_EXPORT int adc_engine_replay_prio_info(adc_engine *e, int32_t member, double *total, float *top)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = per_ready(e)) || (rc = per_member_check(e, member))) return rc;
    ENGINE_GUARD(e);
    const PerView v = per_member(e->per, (size_t)member);
    if (total) HIP_TRY(hipMemcpyAsync(total, v.node[v.levels], sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (top) HIP_TRY(hipMemcpyAsync(top, v.top, sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_replay_prio_fetch(adc_engine *e, int32_t member, int64_t slot, int64_t count, float *leaf)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = per_ready(e)) || (rc = per_member_check(e, member))) return rc;
    if (!leaf) return fail(ADC_EINVAL, "leaf is NULL");
    if (slot < 0 || count < 1 || slot > td3_size(e) - count) return fail(ADC_EINVAL, "the slot range is not inside [0, size)");
    ENGINE_GUARD(e);
    HIP_TRY(hipMemcpyAsync(leaf, per_member(e->per, (size_t)member).leaf + slot, (size_t)count * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_replay_prio_load(adc_engine *e, int32_t member, int64_t slot, int64_t count, const float *leaf, float top)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = per_ready(e)) || (rc = per_member_check(e, member))) return rc;
    if (!leaf) return fail(ADC_EINVAL, "leaf is NULL");
    if (slot < 0 || count < 1 || slot > td3_size(e) - count) return fail(ADC_EINVAL, "the slot range is not inside [0, size)");
    const float inf = __builtin_inff();
    if (!(top > 0.0f && top < inf)) return fail(ADC_EINVAL, "top must be finite and > 0");
    for (int64_t i = 0; i < count; ++i)
        if (!(leaf[i] > 0.0f && leaf[i] < inf)) return fail(ADC_EINVAL, "a leaf must be finite and > 0");
    ENGINE_GUARD(e);
    const PerView v = per_member(e->per, (size_t)member);
    HIP_TRY(hipMemcpyAsync(v.leaf + slot, leaf, (size_t)count * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(v.top, &top, sizeof(float), hipMemcpyHostToDevice, e->stream));
    per_rebuild_range(e, v, 1, (long long)slot, (long long)count);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_replay_prio_batch(adc_engine *e, int32_t member, int64_t update, int32_t *idx_b, float *weight_b)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = per_ready(e)) || (rc = per_member_check(e, member))) return rc;
    if (update < 0 || update >= 0xFFFFFFFFll) return fail(ADC_EINVAL, "update: 0 to 2^32 - 2");
    if (td3_size(e) == 0) return fail(ADC_ESTATE, "the replay buffer is empty");
    ENGINE_GUARD(e);
    // (the batch buffers are scratch between updates: every update writes them anew before it reads them)
    if ((rc = per_sample_run(e, (uint32_t)update))) return rc;
    const PerView v = per_member(e->per, (size_t)member);
    const size_t B = (size_t)v.B;
    if (idx_b) HIP_TRY(hipMemcpyAsync(idx_b, v.slot, B * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (weight_b) HIP_TRY(hipMemcpyAsync(weight_b, v.w, B * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}
