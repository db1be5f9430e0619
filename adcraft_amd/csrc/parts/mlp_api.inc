// mlp_api.inc - the extern "C" entry points of the learned agent (include/adcraft_engine.h; the kernels are parts/kernel_mlp_policy.inc,
// the law is csrc/adc_mlp.h), over parts/mlp_core.inc: the single policy, one agent per env; policy populations (per-member policy
// layers, parts/kernel_es.inc); learners (per-member policy layers, value layers and log_std, the population trainers' members); the
// squashed action and the bounded act of the single policy or of the learners.
// (part of the single translation unit adc_engine.hip)

// ---- the single policy ---------------------------------------------------------------------------------------------------------------
namespace {
int mlp_init_core(adc_engine *e, const adc_mlp_config *cfg, const uint64_t *seeds_n, int32_t frames, int32_t G);
}
ADC_EXPORT int adc_engine_mlp_init(adc_engine *e, const adc_mlp_config *cfg, const uint64_t *seeds_n) { return adc_engine_mlp_init_frames(e, cfg, seeds_n, 1); }

ADC_EXPORT int adc_engine_mlp_init_frames(adc_engine *e, const adc_mlp_config *cfg, const uint64_t *seeds_n, int32_t frames)
{
    return mlp_init_core(e, cfg, seeds_n, frames, 0);
}

namespace {
// the init under adc_engine_mlp_init_frames (G = 0) and adc_engine_mlp_init_recurrent (frames = 1, G > 0: parts/gru_api.inc has checked G).
// With a cell the policy's layers are the trunk and the output layer [G][P], the cell's two stores are the view's (MlpGruView), and
// the flat order has two more terms - the trunk, Wi | bi, Wh | bh, the output layer (adc_gru.h) - which a population and the strategy
// walk as they walk layers.
int mlp_init_core(adc_engine *e, const adc_mlp_config *cfg, const uint64_t *seeds_n, int32_t frames, int32_t G)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const char *why = nullptr;
    if (adc_mlp_config_check(cfg, e->v.K, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    if (frames < 1 || frames > adc::kMlpMaxFrames) return fail(ADC_EINVAL, "frames: 1 to 8");
    const int K = e->v.K, A = K + 1, D0 = 5 * K + 2, D = frames * D0;
    const int P = cfg->policy_widths[cfg->n_policy_layers - 1];
    if (mlp_lds_floats(D0, P) * sizeof(float) > 150u * 1024u) return fail(ADC_EINVAL, "num_keywords too large for the MLP policy (LDS)");
    if (mlp_lds_floats(D, P) * sizeof(float) > 150u * 1024u)
        return fail(ADC_EINVAL, "frames: the stacked input row is too large for the MLP policy (LDS); fewer frames fit");
    if (G > 0 && mlp_gru_lds_floats(D, P, G) * sizeof(float) > 150u * 1024u)
        return fail(ADC_EINVAL, "gru_width: the cell's state and gates do not fit beside the input row (LDS); a narrower cell fits");
    ENGINE_GUARD(e);
    population_drop(e);                 // (a population does not survive a re-initialisation, as the rollout record does not)
    learners_drop(e);
    pg_drop(e);
    td3_drop(e);
    mlp_free(e, e->mlp_allocs);
    e->have_mlp = false;
    e->gv = MlpGruView{};
    MlpView p{};
    const size_t N = e->v.N;
    int rc;
    auto net = [&](MlpNet &n, int layers, const int32_t *widths, int state_from = adc::kMlpMaxLayers, int state_width = 0) {
        n.layers = layers;
        int n_in = D;
        for (int l = 0; l < layers; ++l) {
            if (l >= state_from) n_in = state_width;        // (Wh and the output layer of a recurrent policy read the state)
            float *w = nullptr, *b = nullptr;
            if ((rc = mlp_alloc(e, e->mlp_allocs, &w, adc::mlp_weight_count(n_in, widths[l]))) || (rc = mlp_alloc(e, e->mlp_allocs, &b, (size_t)widths[l])))
                return rc;
            n.W[l] = w; n.b[l] = b; n.n_in[l] = n_in; n.n_out[l] = widths[l];
            n_in = widths[l];
        }
        return (int)ADC_OK;
    };
    // (with a cell the output layer reads the state)
    const int at = cfg->n_policy_layers - 1;
    if ((rc = net(p.pol, cfg->n_policy_layers, cfg->policy_widths, G > 0 ? at : adc::kMlpMaxLayers, G))) return rc;
    if ((rc = net(p.val, cfg->n_value_layers, cfg->value_widths))) return rc;
    MlpGruView gv{};
    if (G > 0) {
        gv.G = G; gv.at = at; gv.n_in = at > 0 ? cfg->policy_widths[at - 1] : D;
        float *wi = nullptr, *bi = nullptr, *wh = nullptr, *bh = nullptr;
        if ((rc = mlp_alloc(e, e->mlp_allocs, &wi, adc::mlp_weight_count(gv.n_in, 3 * G))) || (rc = mlp_alloc(e, e->mlp_allocs, &bi, (size_t)3 * G)) ||
            (rc = mlp_alloc(e, e->mlp_allocs, &wh, adc::mlp_weight_count(G, 3 * G))) || (rc = mlp_alloc(e, e->mlp_allocs, &bh, (size_t)3 * G)))
            return rc;
        gv.Wi = wi; gv.bi = bi; gv.Wh = wh; gv.bh = bh;
    }
    float *shift = nullptr, *scale = nullptr, *log_std = nullptr;
    if (cfg->normalize) {
        if ((rc = mlp_alloc(e, e->mlp_allocs, &shift, (size_t)D)) || (rc = mlp_alloc(e, e->mlp_allocs, &scale, (size_t)D))) return rc;
    }
    if ((rc = mlp_alloc(e, e->mlp_allocs, &log_std, (size_t)A))) return rc;
    p.shift = shift; p.scale = scale; p.log_std = log_std;
    p.activation = cfg->activation == ADC_MLP_TANH ? adc::kMlpTanh : adc::kMlpRelu;
    p.two_heads = P == 2 * A;
    p.clamp = cfg->clamp_log_std != 0; p.ls_lo = cfg->log_std_lo; p.ls_hi = cfg->log_std_hi;
    p.clip_hi = cfg->bid_clip_hi;
    p.deterministic = cfg->deterministic != 0;
    p.A = A; p.D = D; p.P = P;
    // the flat parameter order, and a member's block: its layers one after the other, each starting on a 16-byte boundary
    // (its terms are the policy's layers; with a cell Wi and Wh stand in front of the output layer, adc_gru.h)
    ParamLayout pl{};
    pl.layers = p.pol.layers + (G > 0 ? 2 : 0);
    for (int t = 0; t < pl.layers; ++t) {
        const int l = G > 0 && t > at ? t - 2 : t;          // (the policy layer of a term that is one)
        if (G > 0 && t == at) { pl.n_in[t] = gv.n_in; pl.n_out[t] = 3 * G; }
        else if (G > 0 && t == at + 1) { pl.n_in[t] = G; pl.n_out[t] = 3 * G; }
        else { pl.n_in[t] = p.pol.n_in[l]; pl.n_out[t] = p.pol.n_out[l]; }
    }
    {
        size_t off = 0;
        int flat = 0;
        for (int l = 0; l < pl.layers; ++l) {
            pl.flat0[l] = flat;
            flat += pl.n_in[l] * pl.n_out[l] + pl.n_out[l];
            pl.offW[l] = (uint32_t)off; off += adc::mlp_weight_count(pl.n_in[l], pl.n_out[l]);
            pl.offb[l] = (uint32_t)off; off += ((size_t)pl.n_out[l] + 3u) & ~(size_t)3u;
            if (G == 0 || l < at) { p.pop_offW[l] = pl.offW[l]; p.pop_offb[l] = pl.offb[l]; }
        }
        if (G > 0) {
            gv.pop_Wi = pl.offW[at]; gv.pop_bi = pl.offb[at]; gv.pop_Wh = pl.offW[at + 1]; gv.pop_bh = pl.offb[at + 1];
            gv.pop_Wo = pl.offW[at + 2]; gv.pop_bo = pl.offb[at + 2];
        }
        pl.P = flat;
        pl.stride = (uint32_t)off;
        e->pl = pl;
        if ((rc = mlp_alloc(e, e->mlp_allocs, &e->mlp_flat, (size_t)flat))) return rc;
    }
    if ((rc = mlp_alloc(e, e->mlp_allocs, &p.key, N)) || (rc = mlp_alloc(e, e->mlp_allocs, &p.tick, N)) ||
        (rc = mlp_alloc(e, e->mlp_allocs, &p.mean, N * A)) || (rc = mlp_alloc(e, e->mlp_allocs, &p.ls, N * A)) ||
        (rc = mlp_alloc(e, e->mlp_allocs, &p.action, N * A)) || (rc = mlp_alloc(e, e->mlp_allocs, &p.logp, N)) ||
        (rc = mlp_alloc(e, e->mlp_allocs, &p.value, N)) || (rc = mlp_alloc(e, e->mlp_allocs, &e->mlp_boot, N)) ||
        (rc = mlp_alloc(e, e->mlp_allocs, &e->mlp_sq, (size_t)2 * A)) || (rc = mlp_alloc(e, e->mlp_allocs, &e->mlp_bd, (size_t)3 * A)))
        return rc;                      // (squash and bounds are off after a re-initialisation: p.sq_lo and p.bd_lo are null)
    e->mlp_bd_host.clear();
    p.frames = frames;
    if (frames > 1 && ((rc = mlp_alloc(e, e->mlp_allocs, &p.hist, N * (size_t)D)) || (rc = mlp_alloc(e, e->mlp_allocs, &p.last, N)) ||
                       (rc = mlp_alloc(e, e->mlp_allocs, &p.from, N))))
        return rc;
    if (G > 0 && ((rc = mlp_alloc(e, e->mlp_allocs, &gv.h, N * 2u * (size_t)G)) || (rc = mlp_alloc(e, e->mlp_allocs, &gv.last, N)) ||
                  (rc = mlp_alloc(e, e->mlp_allocs, &gv.from, N))))
        return rc;
    e->mp = p;
    e->gv = gv;
    e->gru_set = false;
    e->mlp_cfg = *cfg;
    std::memset(e->mlp_layer_set, 0, sizeof(e->mlp_layer_set));
    e->mlp_norm_set = e->mlp_log_std_set = false;
    uint64_t *d_seeds = nullptr;
    hipError_t err = hipSuccess;
    if (seeds_n) {
        HIP_TRY(hipMalloc((void **)&d_seeds, N * 8));
        err = hipMemcpyAsync(d_seeds, seeds_n, N * 8, hipMemcpyHostToDevice, e->stream);
    }
    if (err == hipSuccess) {
        hipLaunchKernelGGL(k_mlp_init, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, e->stream, e->mp, (int)N, d_seeds, e->cfg.seed, e->cfg.env_id_base);
        err = hipGetLastError();
    }
    if (err == hipSuccess && e->mp.hist) {          // no env has acted
        hipLaunchKernelGGL(k_mlp_hist_forget, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, e->stream, (int)N, nullptr, e->mp.last);
        err = hipGetLastError();
    }
    if (err == hipSuccess && e->gv.G) {             // ... and no cell has a state
        hipLaunchKernelGGL(k_mlp_hist_forget, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, e->stream, (int)N, nullptr, e->gv.last);
        err = hipGetLastError();
    }
    const hipError_t err2 = hipStreamSynchronize(e->stream);
    (void)hipFree(d_seeds);
    HIP_TRY(err);
    HIP_TRY(err2);
    e->have_mlp = true;
    // (a record sized for another action width does not survive a re-initialisation)
    if (e->ro_T > 0) { mlp_free(e, e->ro_allocs); e->ro_T = e->ro_t = 0; e->ro_obs = nullptr; e->ro_teacher = e->ro_dagger = 0; e->dg_mask = nullptr; }
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_mlp_set_layer(adc_engine *e, int32_t network, int32_t layer, const float *weights_in_out, const float *bias_out)
{
    if (int rc = mlp_have(e)) return rc;
    if (network != 0 && network != 1) return fail(ADC_EINVAL, "network: 0 (policy) or 1 (value)");
    const MlpNet &n = network == 0 ? e->mp.pol : e->mp.val;
    if (layer < 0 || layer >= n.layers) return fail(ADC_EINVAL, "no such layer");
    if (!weights_in_out || !bias_out) return fail(ADC_EINVAL, "weights or bias is NULL");
    ENGINE_GUARD(e);
    if (int rc = mlp_layer_upload(e, const_cast<float *>(n.W[layer]), const_cast<float *>(n.b[layer]), n.n_in[layer], n.n_out[layer], weights_in_out, bias_out))
        return rc;
    e->mlp_layer_set[network][layer] = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_mlp_set_norm(adc_engine *e, const float *shift_d, const float *scale_d)
{
    if (int rc = mlp_have(e)) return rc;
    if (!e->mp.shift) return fail(ADC_EINVAL, "the policy was initialised without normalisation");
    if (!shift_d || !scale_d) return fail(ADC_EINVAL, "shift or scale is NULL");
    ENGINE_GUARD(e);
    for (const NormSet *s : {&e->on, &e->tn, &e->sn}) {
        if (!s->shared_shift) continue;
        // per-member vectors are in force: every member's row, and the policy's own vectors (the running moments are not touched)
        const size_t D = (size_t)e->mp.D;
        for (int m = 0; m < s->M; ++m) {
            HIP_TRY(hipMemcpyAsync(s->obs.shift + (size_t)m * D, shift_d, D * 4, hipMemcpyHostToDevice, e->stream));
            HIP_TRY(hipMemcpyAsync(s->obs.scale + (size_t)m * D, scale_d, D * 4, hipMemcpyHostToDevice, e->stream));
        }
        HIP_TRY(hipMemcpyAsync(const_cast<float *>(s->shared_shift), shift_d, D * 4, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(const_cast<float *>(s->shared_scale), scale_d, D * 4, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        return ADC_OK;
    }
    HIP_TRY(hipMemcpyAsync(const_cast<float *>(e->mp.shift), shift_d, (size_t)e->mp.D * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(const_cast<float *>(e->mp.scale), scale_d, (size_t)e->mp.D * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->mlp_norm_set = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_mlp_set_log_std(adc_engine *e, const float *log_std_a)
{
    if (int rc = mlp_have(e)) return rc;
    if (!log_std_a) return fail(ADC_EINVAL, "log_std is NULL");
    ENGINE_GUARD(e);
    HIP_TRY(hipMemcpyAsync(const_cast<float *>(e->mp.log_std), log_std_a, (size_t)e->mp.A * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->mlp_log_std_set = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_mlp_set_deterministic(adc_engine *e, int32_t deterministic)
{
    if (int rc = mlp_have(e)) return rc;
    ENGINE_GUARD(e);
    e->mp.deterministic = deterministic != 0;
    e->mlp_cfg.deterministic = deterministic != 0;
    return ADC_OK;
}

namespace {
// the squash of the single policy (learners = false) or of the learners: [lo | half] to the device.  The learners' is one pair for all
// members (k_mlp_policy<2, true>) in the single policy's fields, free while learners are active, and goes with them (learners_drop).
// The two entry points have always refused in different orders - a lone vector first against last - and keep them
int squash_set(adc_engine *e, bool learners, const float *lo_a, const float *hi_a)
{
    if (int rc = mlp_have(e)) return rc;
    if (int rc = gru_refuses(e, "the squashed action")) return rc;
    const bool lone = (lo_a == nullptr) != (hi_a == nullptr);
    if (lone && !learners) return fail(ADC_EINVAL, "lo and hi: both vectors, or both NULL (squash off)");
    if (learners) {
        if (e->lrn_M == 0) return fail(ADC_ESTATE, "the learners' squashed action needs learners (adc_engine_mlp_learners)");
        if (lo_a && e->mp.bd_lo) return fail(ADC_ESTATE, "the squashed action together with the bounded act is not supported (adc_engine_mlp_learners_set_bounds(NULL, NULL) first)");
    } else {
        if (e->pop_M != 0) return fail(ADC_ESTATE, "the squashed action with a population active is not supported (adc_engine_mlp_population(0) first)");
        if (e->lrn_M != 0) return fail(ADC_ESTATE, "the squashed action with learners active is not supported (adc_engine_mlp_learners(0) first)");
        if (lo_a && e->mp.bd_lo) return fail(ADC_ESTATE, "the squashed action together with the bounded act is not supported (adc_engine_mlp_set_bounds(NULL, NULL) first)");
    }
    if (lone) return fail(ADC_EINVAL, "lo and hi: both vectors, or both NULL (squash off)");
    const int A = e->mp.A;
    std::vector<float> v((size_t)2 * A);
    for (int a = 0; lo_a && a < A; ++a) {
        if (!std::isfinite(lo_a[a]) || !std::isfinite(hi_a[a]) || !(hi_a[a] > lo_a[a])) return fail(ADC_EINVAL, "squash bounds: finite, hi > lo");
        v[(size_t)a] = lo_a[a];
        v[(size_t)(A + a)] = adc::mlp_squash_half(lo_a[a], hi_a[a]);
        if (!std::isfinite(v[(size_t)(A + a)])) return fail(ADC_EINVAL, "squash bounds: hi - lo overflows");
    }
    ENGINE_GUARD(e);
    if (!lo_a) { e->mp.sq_lo = e->mp.sq_half = nullptr; return ADC_OK; }
    HIP_TRY(hipMemcpyAsync(e->mlp_sq, v.data(), v.size() * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->mp.sq_lo = e->mlp_sq; e->mp.sq_half = e->mlp_sq + A;
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_mlp_set_squash(adc_engine *e, const float *lo_a, const float *hi_a) { return squash_set(e, false, lo_a, hi_a); }
ADC_EXPORT int adc_engine_mlp_learners_set_squash(adc_engine *e, const float *lo_a, const float *hi_a) { return squash_set(e, true, lo_a, hi_a); }

ADC_EXPORT int adc_engine_mlp_act(adc_engine *e, float budget_override, const float *replay_normals_na)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = mlp_ready(e)) return rc;
    ENGINE_GUARD(e);
    float *d_z = nullptr;
    const size_t na = (size_t)e->v.N * (size_t)e->mp.A;
    hipError_t err = hipSuccess;
    if (replay_normals_na) {
        if (hipMalloc((void **)&d_z, na * 4) != hipSuccess) { (void)hipGetLastError(); return fail(ADC_ENOMEM, "hipMalloc failed"); }
        err = hipMemcpyAsync(d_z, replay_normals_na, na * 4, hipMemcpyHostToDevice, e->stream);
    }
    if (err == hipSuccess) {
        mlp_launch_kernel(e->v, e->mp, e->stream, 0, d_z, budget_override, e->d_bids, e->d_budget, MlpRecordSlot{nullptr, nullptr, nullptr, nullptr}, nullptr,
                          &e->gv);
        err = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(e->stream);
    (void)hipFree(d_z);
    HIP_TRY(err);
    HIP_TRY(e2);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_mlp_step(adc_engine *e, float budget_override)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->have_reset) return fail(ADC_ESTATE, "reset required, need to generate keywords to bid on");
    if (int rc = mlp_ready(e)) return rc;
    ENGINE_GUARD_STEP(e);
    return mlp_day(e, budget_override, /* with_ideal = */ false);
}

ADC_EXPORT int adc_engine_mlp_last(adc_engine *e, float *mean_na, float *log_std_na, float *action_na, float *logp_n, float *value_n)
{
    ENGINE_GUARD(e);
    if (!e->have_mlp) return fail(ADC_ESTATE, "adc_engine_mlp_init has not been called");
    const size_t n = (size_t)e->v.N, na = n * (size_t)e->mp.A;
    if (mean_na) HIP_TRY(hipMemcpyAsync(mean_na, e->mp.mean, na * 4, hipMemcpyDeviceToHost, e->stream));
    if (log_std_na) HIP_TRY(hipMemcpyAsync(log_std_na, e->mp.ls, na * 4, hipMemcpyDeviceToHost, e->stream));
    if (action_na) HIP_TRY(hipMemcpyAsync(action_na, e->mp.action, na * 4, hipMemcpyDeviceToHost, e->stream));
    if (logp_n) HIP_TRY(hipMemcpyAsync(logp_n, e->mp.logp, n * 4, hipMemcpyDeviceToHost, e->stream));
    if (value_n) HIP_TRY(hipMemcpyAsync(value_n, e->mp.value, n * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_mlp_agent_state(adc_engine *e, uint64_t *keys_n, uint32_t *ticks_n)
{
    ENGINE_GUARD(e);
    if (!e->have_mlp) return fail(ADC_ESTATE, "adc_engine_mlp_init has not been called");
    if (keys_n) HIP_TRY(hipMemcpyAsync(keys_n, e->mp.key, (size_t)e->v.N * 8, hipMemcpyDeviceToHost, e->stream));
    if (ticks_n) HIP_TRY(hipMemcpyAsync(ticks_n, e->mp.tick, (size_t)e->v.N * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_mlp_frames(adc_engine *e, int32_t *frames)
{
    ENGINE_GUARD(e);
    if (!e->have_mlp) return fail(ADC_ESTATE, "adc_engine_mlp_init has not been called");
    if (!frames) return fail(ADC_EINVAL, "frames is NULL");
    *frames = mlp_frames(e);
    return ADC_OK;
}

// the observation history to the host and back (any pointer may be NULL); without one (frames = 1) there is nothing to move
ADC_EXPORT int adc_engine_mlp_history_get(adc_engine *e, float *hist_nhd, int32_t *last_n, int32_t *from_n)
{
    ENGINE_GUARD(e);
    if (!e->have_mlp) return fail(ADC_ESTATE, "adc_engine_mlp_init has not been called");
    if (!e->mp.hist) return fail(ADC_ESTATE, "the policy has no observation history (adc_engine_mlp_init_frames, frames > 1)");
    const size_t n = (size_t)e->v.N;
    if (hist_nhd) HIP_TRY(hipMemcpyAsync(hist_nhd, e->mp.hist, n * (size_t)e->mp.D * 4, hipMemcpyDeviceToHost, e->stream));
    if (last_n) HIP_TRY(hipMemcpyAsync(last_n, e->mp.last, n * 4, hipMemcpyDeviceToHost, e->stream));
    if (from_n) HIP_TRY(hipMemcpyAsync(from_n, e->mp.from, n * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_mlp_history_set(adc_engine *e, const float *hist_nhd, const int32_t *last_n, const int32_t *from_n)
{
    ENGINE_GUARD(e);
    if (!e->have_mlp) return fail(ADC_ESTATE, "adc_engine_mlp_init has not been called");
    if (!e->mp.hist) return fail(ADC_ESTATE, "the policy has no observation history (adc_engine_mlp_init_frames, frames > 1)");
    const size_t n = (size_t)e->v.N;
    // (the kernels index the frames by these words: nothing a history cannot hold gets in)
    for (size_t i = 0; i < n; ++i)
        if ((last_n && last_n[i] < adc::kMlpHistNone) || (from_n && from_n[i] < 0)) return fail(ADC_EINVAL, "history: last >= -2 and from >= 0");
    if (hist_nhd) HIP_TRY(hipMemcpyAsync(e->mp.hist, hist_nhd, n * (size_t)e->mp.D * 4, hipMemcpyHostToDevice, e->stream));
    if (last_n) HIP_TRY(hipMemcpyAsync(e->mp.last, last_n, n * 4, hipMemcpyHostToDevice, e->stream));
    if (from_n) HIP_TRY(hipMemcpyAsync(e->mp.from, from_n, n * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_mlp_bootstrap_value(adc_engine *e, float *value_n)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!value_n) return fail(ADC_EINVAL, "value_n is NULL");
    if (int rc = mlp_ready(e)) return rc;
    if (e->mp.val.layers == 0) return fail(ADC_ESTATE, "the policy has no value network");
    ENGINE_GUARD(e);
    mlp_launch_kernel(e->v, e->mp, e->stream, 1, nullptr, 0.0f, e->d_bids, e->d_budget, MlpRecordSlot{nullptr, nullptr, nullptr, nullptr}, e->mlp_boot);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(value_n, e->mlp_boot, (size_t)e->v.N * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

// ---- policy populations: per-member weights of the policy network (parts/kernel_es.inc) ---------------------------------------
ADC_EXPORT int adc_engine_mlp_population(adc_engine *e, int32_t members, const int32_t *member_of_env_n)
{
    if (int rc = mlp_have(e)) return rc;
    const int N = e->v.N, M = members;
    if (M < 0 || M > 65536) return fail(ADC_EINVAL, "members: 0 (off) to 65536");
    // (the single policy's squash: the learners' own, on only while they are active, goes with them below)
    if (M > 0 && e->mp.sq_lo && e->lrn_M == 0)
        return fail(ADC_ESTATE, "a population with the squashed action on is not supported (adc_engine_mlp_set_squash(NULL, NULL) first)");
    if (M > 0 && e->mp.bd_lo)
        return fail(ADC_ESTATE, "a population with the bounded act on is not supported: it would need a log-probability (adc_engine_mlp_set_bounds(NULL, NULL) first)");
    std::vector<int32_t> map((size_t)N), count((size_t)M, 0);
    if (M > 0) {
        if (!member_of_env_n && N % M != 0) return fail(ADC_EINVAL, "members must divide num_envs when no member_of_env map is given");
        for (int env = 0; env < N; ++env) {
            const int32_t m = member_of_env_n ? member_of_env_n[env] : env / (N / M);
            if (m < 0 || m >= M) return fail(ADC_EINVAL, "member_of_env names a member outside [0, members)");
            map[(size_t)env] = m;
            count[(size_t)m] += 1;
        }
    }
    ENGINE_GUARD(e);
    if (M == 0) { population_drop(e); return ADC_OK; }      // (learners, if any, stay: there is no population to turn off then)
    // (the new population is allocated before the old one goes: a failure leaves the engine as it was)
    void *block = nullptr, *d_map = nullptr;
    if (hipMalloc(&block, (size_t)M * e->pl.stride * 4) != hipSuccess || hipMalloc(&d_map, (size_t)N * 4) != hipSuccess) {
        (void)hipGetLastError();
        if (block) (void)hipFree(block);
        return fail(ADC_ENOMEM, "hipMalloc failed (policy population)");
    }
    learners_drop(e);                   // (the two kinds of members exclude each other)
    population_drop(e);
    e->pop_allocs.push_back(block);
    e->pop_allocs.push_back(d_map);
    HIP_TRY(hipMemsetAsync(block, 0, (size_t)M * e->pl.stride * 4, e->stream));       // (the never-read padding too)
    HIP_TRY(hipMemcpyAsync(d_map, map.data(), (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
    // every member starts as the centre
    hipLaunchKernelGGL(k_params_copy, dim3((unsigned)((e->pl.P + kEsBlock - 1) / kEsBlock)), dim3(kEsBlock), 0, e->stream, e->pl, centre_store(e),
                       e->mlp_flat, 1);
    hipLaunchKernelGGL(k_es_perturb, dim3(es_quad_blocks(e->pl.P), (unsigned)((M + 1) / 2)), dim3(kEsBlock), 0, e->stream, e->pl, e->mlp_flat,
                       static_cast<float *>(block), (size_t)e->pl.stride, M, 0, (uint64_t)0, 0u, 0.0f);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->mp.member = static_cast<const int32_t *>(d_map);
    e->mp.pop = static_cast<const float *>(block);
    e->mp.pop_stride = e->pl.stride;
    e->pop_M = M;
    e->pop_map.swap(map);
    e->pop_count.swap(count);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_mlp_set_member_layer(adc_engine *e, int32_t member, int32_t layer, const float *weights_in_out, const float *bias_out)
{
    if (int rc = mlp_have(e)) return rc;
    if (int rc = population_member_check(e, member)) return rc;
    if (layer < 0 || layer >= e->mp.pol.layers) return fail(ADC_EINVAL, "no such layer");
    layer = policy_term(e, layer);      // (a member's stores are the flat order's terms: a recurrent policy's output layer stands behind the cell's two)
    if (!weights_in_out || !bias_out) return fail(ADC_EINVAL, "weights or bias is NULL");
    ENGINE_GUARD(e);
    const ParamStore s = member_store(e, member);
    return mlp_layer_upload(e, s.W[layer], s.b[layer], e->pl.n_in[layer], e->pl.n_out[layer], weights_in_out, bias_out);
}

ADC_EXPORT int adc_engine_mlp_param_count(adc_engine *e, int64_t *count)
{
    if (!e || !count) return fail(ADC_EINVAL, "engine handle or count is NULL");
    if (!e->have_mlp) return fail(ADC_ESTATE, "adc_engine_mlp_init has not been called");
    *count = e->pl.P;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_mlp_get_params(adc_engine *e, float *flat_p)
{
    if (int rc = mlp_have(e)) return rc;
    if (!flat_p) return fail(ADC_EINVAL, "flat_p is NULL");
    ENGINE_GUARD(e);
    return params_fetch(e, centre_store(e), flat_p);
}

ADC_EXPORT int adc_engine_mlp_get_member_params(adc_engine *e, int32_t member, float *flat_p)
{
    if (int rc = mlp_have(e)) return rc;
    if (int rc = population_member_check(e, member)) return rc;
    if (!flat_p) return fail(ADC_EINVAL, "flat_p is NULL");
    ENGINE_GUARD(e);
    return params_fetch(e, member_store(e, member), flat_p);
}

// ---- learners: per-member policy layers, value layers and log_std (the population trainer's members; parts/pg_api.inc) ----------
ADC_EXPORT int adc_engine_mlp_learners(adc_engine *e, int32_t members)
{
    if (int rc = mlp_have(e)) return rc;
    if (members > 0)
        if (int rc = gru_refuses(e, "learners")) return rc;
    const int N = e->v.N, M = members;
    if (M < 0 || M > 65535) return fail(ADC_EINVAL, "members: 0 (off) to 65535");
    if (M > 0 && N % M != 0) return fail(ADC_EINVAL, "members must divide num_envs");
    // (the single policy's squash: the learners' own, on only while they are active, goes with them below)
    if (M > 0 && e->mp.sq_lo && e->lrn_M == 0)
        return fail(ADC_ESTATE, "learners with the squashed action on are not supported (adc_engine_mlp_set_squash(NULL, NULL) first)");
    if (M > 0 && e->mp.bd_lo && e->lrn_M == 0)
        return fail(ADC_ESTATE, "learners with the single policy's bounded act on are not supported (adc_engine_mlp_set_bounds(NULL, NULL) first)");
    ENGINE_GUARD(e);
    if (M == 0) { learners_drop(e); return ADC_OK; }
    // the flat order against the centre's stores; a member's block holds the same terms - the policy layers, the value layers, log_std -
    // each W and b starting on a 16-byte boundary, `at` floats from the member's base
    const PgLayout centre = centre_layout(e);
    size_t at[2][adc::kPgMaxTerms] = {}, stride = 0;
    for (int i = 0; i < centre.nterms; ++i) {
        at[0][i] = stride; stride += adc::mlp_weight_count(centre.n_in[i], centre.n_out[i]);        // (none for log_std: n_in = 0)
        at[1][i] = stride; stride += ((size_t)centre.n_out[i] + 3u) & ~(size_t)3u;
    }
    // (the new members are allocated before the old ones go: a failure leaves the engine as it was)
    std::vector<void *> fresh;
    float *block = nullptr, *flat = nullptr;
    int32_t *d_map = nullptr;
    MlpLearner *d_tab = nullptr;
    int rc;
    if ((rc = mlp_alloc(e, fresh, &block, (size_t)M * stride)) || (rc = mlp_alloc(e, fresh, &flat, (size_t)centre.Q)) ||
        (rc = mlp_alloc(e, fresh, &d_map, (size_t)N)) || (rc = mlp_alloc(e, fresh, &d_tab, (size_t)M))) {
        mlp_free(e, fresh);
        return rc;
    }
    population_drop(e);                 // (the two kinds of members exclude each other)
    learners_drop(e);
    e->lrn_allocs.swap(fresh);
    PgLayout lay = centre;              // (member 0's stores; member m's are m * stride floats on)
    for (int i = 0; i < lay.nterms; ++i) { lay.W[i] = centre.W[i] ? block + at[0][i] : nullptr; lay.b[i] = block + at[1][i]; }
    std::vector<MlpLearner> tab((size_t)M);
    for (size_t m = 0; m < (size_t)M; ++m) {
        tab[m].net[0] = e->mp.pol; tab[m].net[1] = e->mp.val;       // (the shapes; the stores are the member's own)
        int i = 0;
        for (int net = 0; net < 2; ++net)
            for (int l = 0; l < tab[m].net[net].layers; ++l, ++i) { tab[m].net[net].W[l] = lay.W[i] + m * stride; tab[m].net[net].b[l] = lay.b[i] + m * stride; }
        tab[m].log_std = e->mp.two_heads ? nullptr : lay.b[i] + m * stride;
    }
    std::vector<int32_t> map((size_t)N);
    for (int env = 0; env < N; ++env) map[(size_t)env] = env / (N / M);
    HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), (size_t)M * sizeof(MlpLearner), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(d_map, map.data(), (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
    // every member starts as the centre: the centre's stores to the flat order, the flat order to every member's stores
    hipLaunchKernelGGL(k_pg_params_copy, dim3(pg_blocks(lay.Q)), dim3(kPgBlock), 0, e->stream, centre, flat, 1);
    hipLaunchKernelGGL(k_pg_pop_params_copy, dim3(pg_blocks(lay.Q), (unsigned)M), dim3(kPgBlock), 0, e->stream, lay, stride, 0, flat, (size_t)0, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));       // (tab and map are the host's until here)
    e->lrn_M = M; e->lrn_n = N / M;
    e->lrn_block = block; e->lrn_flat = flat; e->lrn_stride = stride; e->lrn_tab = d_tab; e->lrn_lay = lay;
    e->mp.member = d_map; e->mp.learners = d_tab; e->mp.pop_stride = 0;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_mlp_set_learner_layer(adc_engine *e, int32_t member, int32_t network, int32_t layer, const float *weights_in_out,
                                                const float *bias_out)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = learners_ready(e, member)) return rc;
    if (network != 0 && network != 1) return fail(ADC_EINVAL, "network: 0 (policy) or 1 (value)");
    const MlpNet &n = network == 0 ? e->mp.pol : e->mp.val;
    if (layer < 0 || layer >= n.layers) return fail(ADC_EINVAL, "no such layer");
    if (!weights_in_out || !bias_out) return fail(ADC_EINVAL, "weights or bias is NULL");
    ENGINE_GUARD(e);
    const int term = (network == 0 ? 0 : e->mp.pol.layers) + layer;
    const size_t base = (size_t)member * e->lrn_stride;
    return mlp_layer_upload(e, e->lrn_lay.W[term] + base, e->lrn_lay.b[term] + base, n.n_in[layer], n.n_out[layer], weights_in_out, bias_out);
}

ADC_EXPORT int adc_engine_mlp_set_learner_log_std(adc_engine *e, int32_t member, const float *log_std_a)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = learners_ready(e, member)) return rc;
    if (e->mp.two_heads) return fail(ADC_EINVAL, "a two-headed policy has no log_std vector");
    if (!log_std_a) return fail(ADC_EINVAL, "log_std is NULL");
    ENGINE_GUARD(e);
    float *dst = e->lrn_lay.b[e->lrn_lay.nterms - 1] + (size_t)member * e->lrn_stride;
    HIP_TRY(hipMemcpyAsync(dst, log_std_a, (size_t)e->mp.A * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_mlp_get_learner_params(adc_engine *e, int32_t member, float *theta_q)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = learners_ready(e, member)) return rc;
    if (!theta_q) return fail(ADC_EINVAL, "theta_q is NULL");
    ENGINE_GUARD(e);
    const int Q = e->lrn_lay.Q;
    hipLaunchKernelGGL(k_pg_pop_params_copy, dim3(pg_blocks(Q), 1u), dim3(kPgBlock), 0, e->stream, e->lrn_lay, e->lrn_stride, (int)member, e->lrn_flat,
                       (size_t)0, 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(theta_q, e->lrn_flat, (size_t)Q * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

// ---- the bounded act (the law is adc_mlp.h "bounded"; bounded TD3 over it is parts/td3_bounded_api.inc) ------------------------------
namespace {
// the bounds of the single policy (learners = false) or of the learners: [lo | half | 1 / half] to the device, lo and hi kept on the host
int bounds_set(adc_engine *e, bool learners, const float *lo_a, const float *hi_a)
{
    if (int rc = mlp_have(e)) return rc;
    if (int rc = gru_refuses(e, "the bounded act")) return rc;
    if ((lo_a == nullptr) != (hi_a == nullptr)) return fail(ADC_EINVAL, "lo and hi: both vectors, or both NULL (bounds off)");
    if (learners) {
        if (e->lrn_M == 0) return fail(ADC_ESTATE, "the learners' bounded act needs learners (adc_engine_mlp_learners)");
    } else {
        if (e->pop_M != 0) return fail(ADC_ESTATE, "the bounded act with a population active is not supported (adc_engine_mlp_population(0) first)");
        if (e->lrn_M != 0) return fail(ADC_ESTATE, "learners are active: their bounds are set through adc_engine_mlp_learners_set_bounds");
    }
    if (lo_a && e->mp.sq_lo)
        return fail(ADC_ESTATE, "the bounded act together with the squashed action is not supported (adc_engine_mlp_set_squash(NULL, NULL) first)");
    if (lo_a && e->mp.two_heads)
        return fail(ADC_ESTATE, "the bounded act needs the policy with the free log_std head: a two-headed policy (2A outputs) is not supported");
    if ((e->have_td3 || e->have_td3_pop) && e->td3_written > 0)
        return fail(ADC_ESTATE, "the replay ring holds transitions: their actions are in units of the bounds as they are, which may not change "
                                "(a new adc_engine_td3_init / adc_engine_td3_pop_init starts an empty ring)");
    const int A = e->mp.A;
    std::vector<float> v((size_t)3 * A);
    for (int a = 0; lo_a && a < A; ++a) {
        if (!std::isfinite(lo_a[a]) || !std::isfinite(hi_a[a]) || !(hi_a[a] > lo_a[a])) return fail(ADC_EINVAL, "action bounds: finite, hi > lo");
        const float half = adc::mlp_squash_half(lo_a[a], hi_a[a]), inv = adc::mlp_inv_half(half);
        if (!std::isfinite(half) || !(half > 0.0f) || !std::isfinite(inv)) return fail(ADC_EINVAL, "action bounds: hi - lo overflows or vanishes");
        v[(size_t)a] = lo_a[a]; v[(size_t)(A + a)] = half; v[(size_t)(2 * A + a)] = inv;
    }
    ENGINE_GUARD(e);
    if (!lo_a) {
        e->mp.bd_lo = e->mp.bd_half = nullptr;
        e->mp.explore = adc::kMlpGaussian;      // (the random mode is the bounded act's alone)
        e->mlp_bd_host.clear();
        return ADC_OK;
    }
    HIP_TRY(hipMemcpyAsync(e->mlp_bd, v.data(), v.size() * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->mp.bd_lo = e->mlp_bd; e->mp.bd_half = e->mlp_bd + A;
    e->mlp_bd_host.assign(lo_a, lo_a + A);
    e->mlp_bd_host.insert(e->mlp_bd_host.end(), hi_a, hi_a + A);
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_mlp_set_bounds(adc_engine *e, const float *lo_a, const float *hi_a) { return bounds_set(e, false, lo_a, hi_a); }
ADC_EXPORT int adc_engine_mlp_learners_set_bounds(adc_engine *e, const float *lo_a, const float *hi_a) { return bounds_set(e, true, lo_a, hi_a); }

ADC_EXPORT int adc_engine_mlp_set_explore(adc_engine *e, int32_t mode)
{
    if (int rc = mlp_have(e)) return rc;
    if (mode != ADC_MLP_EXPLORE_GAUSSIAN && mode != ADC_MLP_EXPLORE_RANDOM) return fail(ADC_EINVAL, "unknown exploration mode");
    if (mode == ADC_MLP_EXPLORE_RANDOM && !e->mp.bd_lo)
        return fail(ADC_ESTATE, "the random exploration mode needs the bounded act: actions are drawn uniformly from its box (adc_engine_mlp_set_bounds)");
    ENGINE_GUARD(e);
    e->mp.explore = mode == ADC_MLP_EXPLORE_RANDOM ? adc::kMlpRandom : adc::kMlpGaussian;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_mlp_get_bounds(adc_engine *e, float *lo_a, float *hi_a, int32_t *bounded, int32_t *explore)
{
    if (int rc = mlp_have(e)) return rc;
    const bool on = e->mp.bd_lo != nullptr;
    const size_t A = (size_t)e->mp.A;
    if (on && lo_a) std::copy(e->mlp_bd_host.begin(), e->mlp_bd_host.begin() + (long)A, lo_a);
    if (on && hi_a) std::copy(e->mlp_bd_host.begin() + (long)A, e->mlp_bd_host.end(), hi_a);
    if (bounded) *bounded = on ? 1 : 0;
    if (explore) *explore = e->mp.explore == adc::kMlpRandom ? ADC_MLP_EXPLORE_RANDOM : ADC_MLP_EXPLORE_GAUSSIAN;
    return ADC_OK;
}
