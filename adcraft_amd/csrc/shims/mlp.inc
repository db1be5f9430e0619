// mlp.inc (part of adc_shims.cpp) - the MLP policy on the host (adc_mlp.h: the code parts/kernel_mlp_policy.inc runs) and the recurrent policy (adc_gru.h:
// the code parts/kernel_mlp_gru.inc runs)
// the checks adc_engine_mlp_init makes on a configuration for an engine of num_keywords keywords; message (nullable) names the first failure
ADC_EXPORT int adc_mlp_config_check(const adc_mlp_config *cfg, int32_t num_keywords, const char **message)
{
    const char *msg = nullptr;
    const int A = num_keywords + 1;
    if (!cfg || cfg->struct_size != sizeof(adc_mlp_config)) msg = "adc_mlp_config: NULL or struct_size mismatch";
    else if (num_keywords < 1) msg = "num_keywords < 1";
    else if (cfg->activation != ADC_MLP_TANH && cfg->activation != ADC_MLP_RELU) msg = "unknown activation";
    else if (cfg->n_policy_layers < 1 || cfg->n_policy_layers > adc::kMlpMaxLayers) msg = "the policy network has 1 to 4 layers";
    else if (cfg->n_value_layers < 0 || cfg->n_value_layers > adc::kMlpMaxLayers) msg = "the value network has 0 to 4 layers";
    else if (cfg->clamp_log_std && !(cfg->log_std_lo <= cfg->log_std_hi)) msg = "log_std clamp: lo <= hi";
    else {
        for (int l = 0; l + 1 < cfg->n_policy_layers && !msg; ++l)
            if (cfg->policy_widths[l] < 1 || cfg->policy_widths[l] > adc::kMlpMaxWidth) msg = "hidden widths are 1 to 256";
        for (int l = 0; l + 1 < cfg->n_value_layers && !msg; ++l)
            if (cfg->value_widths[l] < 1 || cfg->value_widths[l] > adc::kMlpMaxWidth) msg = "hidden widths are 1 to 256";
        const int P = cfg->policy_widths[cfg->n_policy_layers - 1];
        if (!msg && P != A && P != 2 * A) msg = "the policy network ends in num_keywords + 1 outputs (means) or twice that (means, log-stds)";
        if (!msg && cfg->n_value_layers > 0 && cfg->value_widths[cfg->n_value_layers - 1] != 1) msg = "the value network ends in one output";
    }
    return config_verdict(msg, message);
}

namespace {
// one network of the law on a host input row; weights given [n_in][n_out] row-major, re-laid chain-major as the device holds them
std::vector<float> mlp_forward_host(const float *x0, int D, int layers, const int32_t *widths, const float *const *w, const float *const *b, int activation)
{
    std::vector<float> x(x0, x0 + D);
    for (int l = 0; l < layers; ++l) {
        const int n_in = (int)x.size(), n_out = widths[l];
        std::vector<float> cm(adc::mlp_weight_count(n_in, n_out), 0.0f), y((size_t)n_out);
        for (int j = 0; j < n_in; ++j)
            for (int h = 0; h < n_out; ++h) cm[adc::mlp_weight_index(j, h, n_out)] = w[l][(size_t)j * n_out + h];
        const float *xp = x.data();
        for (int h = 0; h < n_out; ++h) {
            const float v = adc::mlp_neuron(cm.data(), b[l], n_in, n_out, h, [&](int j) { return xp[j]; });
            y[(size_t)h] = l + 1 < layers ? adc::mlp_act(v, activation) : v;
        }
        x.swap(y);
    }
    return x;
}

// what the act and the recurrent act share before the policy network: the checks of their common arguments (false: refused), the
// law's activation, the normalised input row x [D] and the value v of it (0 without a value network)
bool mlp_act_input_host(const adc_mlp_config *cfg, int32_t num_keywords, const float *obs_d, const float *const *policy_w, const float *const *policy_b,
                        const float *const *value_w, const float *const *value_b, const float *shift_d, const float *scale_d, const float *log_std_a,
                        int &activation, std::vector<float> &x, float &v)
{
    if (adc_mlp_config_check(cfg, num_keywords, nullptr) != ADC_OK) return false;
    const int A = num_keywords + 1, D = 5 * num_keywords + 2;
    const bool two_heads = cfg->policy_widths[cfg->n_policy_layers - 1] == 2 * A;
    if (!policy_w || !policy_b || (cfg->n_value_layers > 0 && (!value_w || !value_b)) || (cfg->normalize && (!shift_d || !scale_d)) ||
        (!two_heads && !log_std_a))
        return false;
    activation = cfg->activation == ADC_MLP_TANH ? adc::kMlpTanh : adc::kMlpRelu;
    x.assign((size_t)D, 0.0f);
    for (int j = 0; j < D; ++j) {
        float xj = obs_d ? obs_d[j] : 0.0f;
        if (cfg->normalize) xj = adc::mlp_normalize(xj, shift_d[j], scale_d[j]);
        x[(size_t)j] = xj;
    }
    v = 0.0f;
    if (cfg->n_value_layers > 0) v = mlp_forward_host(x.data(), D, cfg->n_value_layers, cfg->value_widths, value_w, value_b, activation)[0];
    return true;
}

// everything after the policy network's outputs o [P] (adc_mlp.h: heads, sample, log-probability, bids, budget); v: the value
void mlp_heads_host(const adc_mlp_config *cfg, int K, const std::vector<float> &o, float v, const float *log_std_a, const float *normals_a,
                    uint64_t agent_key, uint32_t tick, float budget_override, float *mean_a, float *log_std_out_a, float *action_a, float *logp,
                    float *value, float *bids_k, float *budget)
{
    const int A = K + 1;
    const bool two_heads = cfg->policy_widths[cfg->n_policy_layers - 1] == 2 * A;
    std::vector<float> term((size_t)A);
    for (int a = 0; a < A; ++a) {
        const float mean = o[(size_t)a];
        const float ls = adc::mlp_clamp_log_std(two_heads ? o[(size_t)(A + a)] : log_std_a[a], cfg->clamp_log_std != 0, cfg->log_std_lo, cfg->log_std_hi);
        float z = 0.0f;
        if (!cfg->deterministic) z = normals_a ? normals_a[a] : adc::mlp_normal(agent_key, tick, a);
        const float act = adc::mlp_sample(mean, ls, z, cfg->deterministic != 0);
        if (mean_a) mean_a[a] = mean;
        if (log_std_out_a) log_std_out_a[a] = ls;
        if (action_a) action_a[a] = act;
        if (a == 0) { if (budget) *budget = adc::mlp_budget(act, budget_override); }
        else if (bids_k) bids_k[a - 1] = adc::mlp_bid(act, cfg->bid_clip_hi);
        term[(size_t)a] = adc::mlp_logp_term(z, ls);
    }
    float s[adc::kMlpChains];
    for (int c = 0; c < adc::kMlpChains; ++c) {
        float acc = 0.0f;
        for (int a = c; a < A; a += adc::kMlpChains) acc = acc + term[(size_t)a];
        s[c] = acc;
    }
    if (logp) *logp = adc::mlp_logp_finish(adc::mlp_join8(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]), A);
    if (value) *value = v;
}

// one layer of the law without an activation: y = W x + b, weights [n_in][n_out] row-major
std::vector<float> mlp_linear_host(const float *x, int n_in, int n_out, const float *w, const float *b)
{
    const int32_t widths[1] = {n_out};
    const float *const ws[1] = {w}, *const bs[1] = {b};
    return mlp_forward_host(x, n_in, 1, widths, ws, bs, adc::kMlpTanh);
}
// the cell (adc_gru.h) on x [n_in] and h [G]
std::vector<float> gru_cell_host(int n_in, int G, const float *x, const float *h, const float *wi, const float *bi, const float *wh, const float *bh)
{
    const std::vector<float> gi = mlp_linear_host(x, n_in, 3 * G, wi, bi), gh = mlp_linear_host(h, G, 3 * G, wh, bh);
    std::vector<float> out((size_t)G);
    for (int g = 0; g < G; ++g)
        out[(size_t)g] = adc::gru_unit(gi[(size_t)g], gh[(size_t)g], gi[(size_t)(G + g)], gh[(size_t)(G + g)], gi[(size_t)(2 * G + g)], gh[(size_t)(2 * G + g)], h[g]);
    return out;
}
}  // namespace

ADC_EXPORT int adc_mlp_stack_row_host(int32_t num_keywords, int32_t frames, const float *frame0_d0, float *hist_hd0, int32_t *last, int32_t *from,
                                      int32_t day, int32_t commit, float *row_d)
{
    if (num_keywords < 1 || frames < 1 || frames > adc::kMlpMaxFrames || day < 0 || !hist_hd0 || !last || !from || !row_d) return ADC_EINVAL;
    const int D0 = 5 * num_keywords + 2, D = frames * D0;
    const int32_t fr = adc::mlp_hist_from(day, *last, *from);
    for (int i = 0; i < D; ++i) row_d[i] = i < D0 ? (frame0_d0 && day != 0 ? frame0_d0[i] : 0.0f) : adc::mlp_hist_at(i, D0, frames, hist_hd0, day, fr);
    if (commit) {
        float *slot = hist_hd0 + (size_t)adc::mlp_hist_slot(day, frames) * (size_t)D0;
        for (int j = 0; j < D0; ++j) slot[j] = row_d[j];
        *last = day;
        *from = fr;
    }
    return ADC_OK;
}

ADC_EXPORT int adc_mlp_act_host(const adc_mlp_config *cfg, int32_t num_keywords, const float *obs_d, const float *const *policy_w,
                                const float *const *policy_b, const float *const *value_w, const float *const *value_b, const float *shift_d,
                                const float *scale_d, const float *log_std_a, const float *normals_a, uint64_t agent_key, uint32_t tick,
                                float budget_override, float *mean_a, float *log_std_out_a, float *action_a, float *logp, float *value,
                                float *bids_k, float *budget)
{
    int activation;
    float v;
    std::vector<float> x;
    if (!mlp_act_input_host(cfg, num_keywords, obs_d, policy_w, policy_b, value_w, value_b, shift_d, scale_d, log_std_a, activation, x, v)) return ADC_EINVAL;
    const std::vector<float> o = mlp_forward_host(x.data(), (int)x.size(), cfg->n_policy_layers, cfg->policy_widths, policy_w, policy_b, activation);
    mlp_heads_host(cfg, num_keywords, o, v, log_std_a, normals_a, agent_key, tick, budget_override, mean_a, log_std_out_a, action_a, logp, value, bids_k, budget);
    return ADC_OK;
}

// ---- the recurrent policy on the host (adc_gru.h: the code parts/kernel_mlp_gru.inc runs) ------------------------------------------
ADC_EXPORT int adc_gru_cell_host(int32_t n_in, int32_t gru_width, const float *x_in, const float *h_g, const float *wi_in_3g, const float *bi_3g,
                                 const float *wh_g_3g, const float *bh_3g, float *h_out_g)
{
    if (n_in < 1 || gru_width < 1 || gru_width > adc::kGruMaxWidth || !x_in || !h_g || !wi_in_3g || !bi_3g || !wh_g_3g || !bh_3g || !h_out_g) return ADC_EINVAL;
    const std::vector<float> out = gru_cell_host(n_in, gru_width, x_in, h_g, wi_in_3g, bi_3g, wh_g_3g, bh_3g);
    std::copy(out.begin(), out.end(), h_out_g);
    return ADC_OK;
}

ADC_EXPORT int adc_mlp_act_recurrent_host(const adc_mlp_config *cfg, int32_t num_keywords, int32_t gru_width, const float *obs_d,
                                          const float *const *policy_w, const float *const *policy_b, const float *wi_in_3g, const float *bi_3g,
                                          const float *wh_g_3g, const float *bh_3g, const float *const *value_w, const float *const *value_b,
                                          const float *shift_d, const float *scale_d, const float *log_std_a, const float *normals_a,
                                          uint64_t agent_key, uint32_t tick, float budget_override, const float *h_in_g, float *mean_a,
                                          float *log_std_out_a, float *action_a, float *logp, float *value, float *bids_k, float *budget,
                                          float *h_out_g)
{
    const int G = gru_width;
    int activation;
    float v;
    std::vector<float> x;
    if (!mlp_act_input_host(cfg, num_keywords, obs_d, policy_w, policy_b, value_w, value_b, shift_d, scale_d, log_std_a, activation, x, v)) return ADC_EINVAL;
    if (G < 1 || G > adc::kGruMaxWidth || !wi_in_3g || !bi_3g || !wh_g_3g || !bh_3g) return ADC_EINVAL;
    const int L = cfg->n_policy_layers, P = cfg->policy_widths[L - 1];
    // the trunk (the activation after each of its layers), the cell, the output layer on the new state
    for (int l = 0; l + 1 < L; ++l) {
        std::vector<float> y = mlp_linear_host(x.data(), (int)x.size(), cfg->policy_widths[l], policy_w[l], policy_b[l]);
        for (float &t : y) t = adc::mlp_act(t, activation);
        x.swap(y);
    }
    const std::vector<float> h0((size_t)G, 0.0f);
    const std::vector<float> h1 = gru_cell_host((int)x.size(), G, x.data(), h_in_g ? h_in_g : h0.data(), wi_in_3g, bi_3g, wh_g_3g, bh_3g);
    if (h_out_g) std::copy(h1.begin(), h1.end(), h_out_g);
    const std::vector<float> o = mlp_linear_host(h1.data(), G, P, policy_w[L - 1], policy_b[L - 1]);
    mlp_heads_host(cfg, num_keywords, o, v, log_std_a, normals_a, agent_key, tick, budget_override, mean_a, log_std_out_a, action_a, logp, value, bids_k, budget);
    return ADC_OK;
}

ADC_EXPORT int adc_gru_state_host(int32_t gru_width, int32_t day, float *h_2g, int32_t *last, int32_t *from, float *h_in_g, const float *h_new_g)
{
    const int G = gru_width;
    if (G < 1 || G > adc::kGruMaxWidth || day < 0 || !h_2g || !last || !from || !h_in_g) return ADC_EINVAL;
    const int32_t fr = adc::mlp_hist_from(day, *last, *from);
    const bool zeros = adc::gru_starts_from_zeros(day, fr);
    for (int g = 0; g < G; ++g) h_in_g[g] = zeros ? 0.0f : h_2g[(size_t)adc::gru_read_slot(day) * (size_t)G + (size_t)g];
    if (h_new_g) {
        for (int g = 0; g < G; ++g) h_2g[(size_t)adc::gru_write_slot(day) * (size_t)G + (size_t)g] = h_new_g[g];
        *last = day;
        *from = fr;
    }
    return ADC_OK;
}

ADC_EXPORT float adc_mlp_math_host(int32_t fn, float x) { return fn == 0 ? adc::mlp_tanh(x) : adc::mlp_exp(x); }

ADC_EXPORT int adc_mlp_squash_host(int32_t count, const float *u_a, const float *lo_a, const float *hi_a, float *out_a)
{
    if (count < 0 || (count > 0 && (!u_a || !lo_a || !hi_a || !out_a))) return ADC_EINVAL;
    for (int a = 0; a < count; ++a) out_a[a] = adc::mlp_squash(u_a[a], lo_a[a], adc::mlp_squash_half(lo_a[a], hi_a[a]));
    return ADC_OK;
}

ADC_EXPORT int adc_mlp_bounded_host(int32_t count, const float *mean_a, const float *log_std_a, const float *normals_a, uint64_t agent_key, uint32_t tick,
                                    int32_t mode, const float *lo_a, const float *hi_a, float *n_a, float *env_a)
{
    if (count < 1 || !mean_a || !log_std_a || !lo_a || !hi_a || mode < 0 || mode > 2) return ADC_EINVAL;
    const int deterministic = mode == 1, explore = mode == 2 ? adc::kMlpRandom : adc::kMlpGaussian;
    for (int a = 0; a < count; ++a) {
        float z = 0.0f;
        uint32_t w = 0u;
        if (!deterministic) {
            if (explore == adc::kMlpRandom) w = adc::mlp_word(agent_key, tick, a);
            else z = normals_a ? normals_a[a] : adc::mlp_normal(agent_key, tick, a);
        }
        const float n = adc::mlp_bounded_action(mean_a[a], log_std_a[a], z, w, deterministic, explore);
        if (n_a) n_a[a] = n;
        if (env_a) env_a[a] = adc::mlp_box(n, lo_a[a], adc::mlp_squash_half(lo_a[a], hi_a[a]));
    }
    return ADC_OK;
}

ADC_EXPORT int adc_mlp_unbox_host(int32_t count, const float *e_a, const float *lo_a, const float *hi_a, float *n_a)
{
    if (count < 1 || !e_a || !lo_a || !hi_a || !n_a) return ADC_EINVAL;
    for (int a = 0; a < count; ++a) n_a[a] = adc::mlp_unbox(e_a[a], lo_a[a], adc::mlp_inv_half(adc::mlp_squash_half(lo_a[a], hi_a[a])));
    return ADC_OK;
}

ADC_EXPORT uint64_t adc_mlp_agent_key_host(uint64_t seed) { return adc::mlp_agent_key(seed); }
ADC_EXPORT uint64_t adc_mlp_default_agent_key_host(uint64_t engine_seed, uint64_t global_env_id) { return adc::mlp_default_agent_key(engine_seed, global_env_id); }

ADC_EXPORT int64_t adc_mlp_math_sweep_host(int32_t fn, float lo, float hi, double *out3, int64_t *violations4)
{
    if (!(lo <= hi) || (fn != 0 && fn != 1)) return -1;
    // floats in value order: key = bits of a positive float, or the negation of a negative one's magnitude bits
    auto key_of = [](float f) { const uint32_t u = adc::float_to_bits(f); return (u & 0x80000000u) ? -(int64_t)(u & 0x7FFFFFFFu) : (int64_t)u; };
    auto float_of = [](int64_t k) { return adc::bits_to_float(k < 0 ? (0x80000000u | (uint32_t)(-k)) : (uint32_t)k); };
    const int64_t k0 = key_of(lo), k1 = key_of(hi), total = k1 - k0 + 1;
    const int T = 8;
    struct Part { double max_abs = 0.0, max_ulp = 0.0, max_mag = 0.0; int64_t bad[4] = {0, 0, 0, 0}; };
    std::vector<Part> parts((size_t)T);
    std::vector<std::thread> threads;
    auto eval = [fn](float x) { return fn == 0 ? adc::mlp_tanh(x) : adc::mlp_exp(x); };
    for (int t = 0; t < T; ++t) {
        threads.emplace_back([&, t]() {
            Part &p = parts[(size_t)t];
            const int64_t a = k0 + total * t / T, b = k0 + total * (t + 1) / T;      // keys [a, b); the first compares with its predecessor
            float prev = a > k0 ? eval(float_of(a - 1)) : -__builtin_inff();
            for (int64_t k = a; k < b; ++k) {
                if (k == 0 && a != 0) continue;                                       // (-0 and +0 share key 0: taken once)
                const float x = float_of(k);
                const float y = eval(x);
                const double exact = fn == 0 ? std::tanh((double)x) : std::exp((double)x);
                const double err = std::fabs((double)y - exact);
                if (err > p.max_abs) p.max_abs = err;
                int ex;
                (void)std::frexp(exact, &ex);
                const double ulp = std::ldexp(1.0, std::max(ex - 24, -149));
                if (err / ulp > p.max_ulp) p.max_ulp = err / ulp;
                if (std::fabs((double)y) > p.max_mag) p.max_mag = std::fabs((double)y);
                if (fn == 0 && eval(-x) != -y) p.bad[0] += 1;
                if (y < prev) p.bad[1] += 1;
                if (fn == 0 && std::fabs(y) > 1.0f) p.bad[2] += 1;
                if (y != y) p.bad[3] += 1;
                prev = y;
            }
        });
    }
    for (auto &th : threads) th.join();
    Part all;
    for (const Part &p : parts) {
        all.max_abs = std::max(all.max_abs, p.max_abs); all.max_ulp = std::max(all.max_ulp, p.max_ulp); all.max_mag = std::max(all.max_mag, p.max_mag);
        for (int i = 0; i < 4; ++i) all.bad[i] += p.bad[i];
    }
    if (out3) { out3[0] = all.max_abs; out3[1] = all.max_ulp; out3[2] = all.max_mag; }
    if (violations4) for (int i = 0; i < 4; ++i) violations4[i] = all.bad[i];
    return total;
}
