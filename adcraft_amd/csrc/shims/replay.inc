// replay.inc (part of adc_shims.cpp) - the replay ring's add-ons on the host: prioritised replay, n-step returns
// ---- prioritised replay on the host (adc_per.h: the code parts/kernel_per.inc runs) ----------------------------------------------
ADC_EXPORT int adc_replay_prio_config_check(const adc_replay_prio_config *cfg, const char **message)
{
    const char *msg = nullptr;
    const float inf = __builtin_inff();
    if (!cfg || cfg->struct_size != sizeof(adc_replay_prio_config)) msg = "adc_replay_prio_config: NULL or struct_size mismatch";
    else if (!(cfg->alpha >= 0.0f && cfg->alpha <= 1.0f)) msg = "alpha must be in [0, 1]";
    else if (!(cfg->beta >= 0.0f && cfg->beta <= 1.0f)) msg = "beta must be in [0, 1]";
    else if (!(cfg->eps > 0.0f && cfg->eps < inf)) msg = "eps must be finite and > 0";
    else if (!(cfg->cap > cfg->eps && cfg->cap < inf)) msg = "cap must be finite and > eps";
    return config_verdict(msg, message);
}

static bool per_tree_of(adc::PerTree &t, int64_t capacity, const float *leaf_c)
{
    for (int64_t i = 0; i < capacity; ++i) {
        if (!(leaf_c[i] >= 0.0f && leaf_c[i] < __builtin_inff())) return false;
        t.leaf[(size_t)i] = leaf_c[i];
    }
    t.rebuild();
    return true;
}

ADC_EXPORT int adc_per_tree_host(int64_t capacity, const float *leaf_c, double *nodes, int64_t *counts)
{
    if (capacity < 1 || capacity > (int64_t)1 << 31 || !leaf_c) return ADC_EINVAL;
    adc::PerTree t(capacity);
    if (!per_tree_of(t, capacity, leaf_c)) return ADC_EINVAL;
    if (counts)
        for (int l = 0; l <= adc::kPerMaxLevels; ++l) counts[l] = l <= t.sh.levels ? t.sh.n[l] : 0;
    if (nodes)
        for (int l = 1; l <= t.sh.levels; ++l)
            for (int64_t i = 0; i < t.sh.n[l]; ++i) *nodes++ = t.node[l][(size_t)i];
    return t.sh.levels;
}

ADC_EXPORT int adc_per_descend_host(int64_t capacity, const float *leaf_c, double m, int64_t *slot)
{
    if (capacity < 1 || capacity > (int64_t)1 << 31 || !leaf_c || !slot) return ADC_EINVAL;
    adc::PerTree t(capacity);
    if (!per_tree_of(t, capacity, leaf_c)) return ADC_EINVAL;
    *slot = t.descend(m);
    return ADC_OK;
}

ADC_EXPORT int adc_per_sample_host(const adc_replay_prio_config *cfg, int64_t capacity, int64_t size, const float *leaf_c, uint64_t seed, int64_t update,
                                   int32_t count, int32_t *idx_b, float *weight_b)
{
    if (adc_replay_prio_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    if (capacity < 1 || capacity > (int64_t)1 << 31 || size < 1 || size > capacity || !leaf_c || count < 1 || update < 0 || update >= 0xFFFFFFFFll)
        return ADC_EINVAL;
    adc::PerTree t(capacity);
    if (!per_tree_of(t, capacity, leaf_c)) return ADC_EINVAL;
    const uint64_t key = adc::td3_key(seed);
    std::vector<int64_t> slots((size_t)count);
    float lmin = __builtin_inff();
    for (int32_t b = 0; b < count; ++b) {
        const double m = adc::per_u53(key, (uint32_t)b, (uint32_t)update) * t.total();
        int64_t s = t.descend(m);
        if (s >= size) s = size - 1;
        slots[(size_t)b] = s;
        const float lf = t.leaf[(size_t)s];
        lmin = lf < lmin ? lf : lmin;
    }
    for (int32_t b = 0; b < count; ++b) {
        if (idx_b) idx_b[b] = (int32_t)slots[(size_t)b];
        if (weight_b) weight_b[b] = adc::per_weight(lmin, t.leaf[(size_t)slots[(size_t)b]], cfg->beta);
    }
    return ADC_OK;
}

ADC_EXPORT int adc_per_priority_host(const adc_replay_prio_config *cfg, int32_t count, const float *d1_b, const float *d2_b, float *pa_b)
{
    if (adc_replay_prio_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    if (count < 1 || !d1_b || !d2_b || !pa_b) return ADC_EINVAL;
    for (int32_t b = 0; b < count; ++b) pa_b[b] = adc::per_pa(adc::per_priority(d1_b[b], d2_b[b], cfg->eps, cfg->cap), cfg->alpha);
    return ADC_OK;
}

ADC_EXPORT int adc_per_leaf_update_host(int64_t capacity, float *leaf_c, float *top, int32_t count, const int32_t *idx_b, const float *pa_b)
{
    if (capacity < 1 || !leaf_c || !top || count < 1 || !idx_b || !pa_b) return ADC_EINVAL;
    for (int32_t b = 0; b < count; ++b)
        if (idx_b[b] < 0 || idx_b[b] >= capacity) return ADC_EINVAL;
    // (as the device: every element writes the largest pa among the elements that drew its slot)
    for (int32_t b = 0; b < count; ++b) {
        float hi = pa_b[b];
        for (int32_t o = 0; o < count; ++o)
            if (idx_b[o] == idx_b[b] && pa_b[o] > hi) hi = pa_b[o];
        leaf_c[idx_b[b]] = hi;
        *top = hi > *top ? hi : *top;
    }
    return ADC_OK;
}

// ---- n-step returns on the host (adc_td3.h "n-step") ------------------------------------------------------------------------------
ADC_EXPORT int adc_replay_nstep_check(int32_t n, const char **message)
{
    const char *msg = (n < 1 || n > adc::kNstepMax) ? "n: 1 to 16 days" : nullptr;
    return config_verdict(msg, message);
}

ADC_EXPORT int adc_replay_nstep_host(int32_t n, float gamma, int32_t T, int32_t N, int32_t t0, int32_t t1, const float *reward, const uint8_t *term,
                                     const uint8_t *trunc, float *R, uint8_t *done, float *gn, int32_t *m)
{
    if (adc_replay_nstep_check(n, nullptr) != ADC_OK) return ADC_EINVAL;
    if (T < 1 || N < 1 || t0 < 0 || t1 <= t0 || t1 > T || !reward || !term || !trunc) return ADC_EINVAL;
    for (int32_t t = t0; t < t1; ++t)
        for (int32_t e = 0; e < N; ++e) {
            const size_t row = (size_t)t * (size_t)N + (size_t)e, s = (size_t)(t - t0) * (size_t)N + (size_t)e;
            const adc::Td3Window w = adc::td3_nstep_window(reward + row, term + row, trunc + row, (size_t)N, t1 - t, n, gamma);
            if (R) R[s] = w.R;
            if (done) done[s] = (uint8_t)w.done;
            if (gn) gn[s] = w.g;
            if (m) m[s] = w.m;
        }
    return ADC_OK;
}

// the targets under n-step returns: norm.inc's loops with the window's own discount per element
ADC_EXPORT int adc_td3_y_nstep_host(const adc_td3_config *td3, int32_t count, const float *r_b, const uint8_t *done_b, const float *q_b, const float *gn_b,
                                    float scale, float clip, float *y_b)
{
    return td3_y_host(td3, count, r_b, done_b, q_b, /* nstep = */ true, gn_b, scale, clip, y_b);
}

ADC_EXPORT int adc_sac_y_nstep_host(const adc_sac_config *sac, int32_t count, const float *r_b, const uint8_t *done_b, const float *q_b, const float *lp_b,
                                    const float *gn_b, float alpha, float scale, float clip, float *y_b)
{
    return sac_y_host(sac, count, r_b, done_b, q_b, lp_b, /* nstep = */ true, gn_b, alpha, scale, clip, y_b);
}
