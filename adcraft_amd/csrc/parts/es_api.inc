// es_api.inc - the extern "C" entry points of the evolution strategy over a policy population (include/adcraft_engine.h; the law is
// csrc/adc_es.h, the kernels are parts/kernel_es.inc), over parts/mlp_core.inc.
// (part of the single translation unit adc_engine.hip)
namespace {
int es_ready(const adc_engine *e)
{
    if (!e->have_es) return fail(ADC_ESTATE, "adc_engine_es_init has not been called");
    return ADC_OK;
}
int es_members_have_envs(const adc_engine *e)
{
    for (int32_t c : e->pop_count)
        if (c == 0) return fail(ADC_EINVAL, "a member of the population has no env: it has no fitness");
    return ADC_OK;
}
// a member's fitness: the float64 mean of its envs' returns, envs ascending (the envs' streams have been joined by the guard)
int es_fitness_fetch(adc_engine *e, double *fitness_m)
{
    const size_t N = (size_t)e->v.N;
    std::vector<double> ret(N);
    HIP_TRY(hipMemcpyAsync(ret.data(), e->es_return, N * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int m = 0; m < e->pop_M; ++m) fitness_m[m] = 0.0;
    for (size_t env = 0; env < N; ++env) fitness_m[e->pop_map[env]] = fitness_m[e->pop_map[env]] + ret[env];
    for (int m = 0; m < e->pop_M; ++m) fitness_m[m] = fitness_m[m] / (double)e->pop_count[(size_t)m];
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_es_init(adc_engine *e, const adc_es_config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const char *why = nullptr;
    if (adc_es_config_check(cfg, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    if (int rc = mlp_ready(e)) return rc;
    if (e->pop_M == 0) return fail(ADC_ESTATE, "the evolution strategy needs a population (adc_engine_mlp_population)");
    if (e->pop_M & 1) return fail(ADC_EINVAL, "the evolution strategy needs an even number of members (antithetic pairs)");
    ENGINE_GUARD(e);
    const size_t P = (size_t)e->pl.P;
    std::vector<void *> fresh;
    float *theta = nullptr, *m = nullptr, *v = nullptr, *grad = nullptr;
    double *du = nullptr, *ret = nullptr;
    int rc;
    if ((rc = mlp_alloc(e, fresh, &theta, P)) || (rc = mlp_alloc(e, fresh, &m, P)) || (rc = mlp_alloc(e, fresh, &v, P)) ||
        (rc = mlp_alloc(e, fresh, &grad, P)) || (rc = mlp_alloc(e, fresh, &du, (size_t)e->pop_M / 2)) ||
        (rc = mlp_alloc(e, fresh, &ret, (size_t)e->v.N))) {
        mlp_free(e, fresh);
        return rc;
    }
    mlp_free(e, e->es_allocs);
    e->es_allocs.swap(fresh);
    e->es_theta = theta; e->es_m = m; e->es_v = v; e->es_grad = grad; e->es_du = du; e->es_return = ret;
    e->es_cfg = *cfg;
    e->es_key = adc::es_key(cfg->seed ? cfg->seed : e->cfg.seed);
    e->es_generation = 0;
    e->es_days = 0;
    e->es_accumulate = false;
    // theta starts as the centre policy
    hipLaunchKernelGGL(k_params_copy, dim3((unsigned)((e->pl.P + kEsBlock - 1) / kEsBlock)), dim3(kEsBlock), 0, e->stream, e->pl, centre_store(e),
                       e->es_theta, 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->have_es = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_es_perturb(adc_engine *e)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = es_ready(e)) return rc;
    ENGINE_GUARD(e);
    hipLaunchKernelGGL(k_es_perturb, dim3(es_quad_blocks(e->pl.P), (unsigned)(e->pop_M / 2)), dim3(kEsBlock), 0, e->stream, e->pl, e->es_theta,
                       const_cast<float *>(e->mp.pop), e->mp.pop_stride, e->pop_M, 1, e->es_key, (uint32_t)e->es_generation, e->es_cfg.sigma);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(e->es_return, 0, (size_t)e->v.N * 8, e->stream));
    if (e->gv.G) {                      // (a cell's state was computed under other weights: every env starts its run anew)
        hipLaunchKernelGGL(k_mlp_hist_forget, dim3((unsigned)((e->v.N + 255) / 256)), dim3(256), 0, e->stream, e->v.N, nullptr, e->gv.last);
        HIP_TRY(hipGetLastError());
    }
    e->es_days = 0;
    e->es_accumulate = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_es_fitness(adc_engine *e, double *fitness_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!fitness_m) return fail(ADC_EINVAL, "fitness_m is NULL");
    if (int rc = es_ready(e)) return rc;
    if (int rc = es_members_have_envs(e)) return rc;
    ENGINE_GUARD(e);
    return es_fitness_fetch(e, fitness_m);
}

ADC_EXPORT int adc_engine_es_update(adc_engine *e, const double *fitness_m, adc_es_stats *stats)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = es_ready(e)) return rc;
    if (int rc = es_members_have_envs(e)) return rc;
    if (!fitness_m && e->es_days == 0) return fail(ADC_EINVAL, "no day has been stepped since adc_engine_es_perturb and no fitness was handed in");
    ENGINE_GUARD(e);
    const int M = e->pop_M;
    const size_t P = (size_t)e->pl.P;
    std::vector<double> fit((size_t)M), du;
    if (fitness_m) std::copy(fitness_m, fitness_m + M, fit.begin());
    else if (int rc = es_fitness_fetch(e, fit.data())) return rc;
    adc::es_shape(e->es_cfg.shaping == ADC_ES_RAW ? adc::kEsRaw : adc::kEsCenteredRank, fit.data(), M, du);
    const uint32_t t = (uint32_t)(e->es_generation + 1);
    adc::EsStep step{};
    step.optimiser = e->es_cfg.optimiser == ADC_ES_SGD ? adc::kEsSgd : adc::kEsAdam;
    step.lr = e->es_cfg.lr; step.beta1 = e->es_cfg.beta1; step.beta2 = e->es_cfg.beta2; step.eps = e->es_cfg.eps; step.l2 = e->es_cfg.l2;
    step.c1 = adc::es_bias_correction(step.beta1, t);
    step.c2 = adc::es_bias_correction(step.beta2, t);
    HIP_TRY(hipMemcpyAsync(e->es_du, du.data(), du.size() * 8, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_es_update, dim3((unsigned)(((e->pl.P + 3) / 4 + kEsUpdQuads - 1) / kEsUpdQuads)), dim3(kEsBlock), 0, e->stream, e->pl, centre_store(e), e->es_theta, e->es_m,
                       e->es_v, e->es_grad, e->es_du, M, e->es_key, (uint32_t)e->es_generation, e->es_cfg.sigma, step);
    HIP_TRY(hipGetLastError());
    std::vector<float> g(P), th(P);
    HIP_TRY(hipMemcpyAsync(g.data(), e->es_grad, P * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(th.data(), e->es_theta, P * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->es_generation += 1;
    e->es_accumulate = false;
    e->es_days = 0;
    if (stats) {
        double sum = 0.0, mx = fit[0], mn = fit[0], gg = 0.0, tt = 0.0;
        for (double f : fit) { sum += f; mx = f > mx ? f : mx; mn = f < mn ? f : mn; }
        for (size_t p = 0; p < P; ++p) { gg += (double)g[p] * (double)g[p]; tt += (double)th[p] * (double)th[p]; }
        stats->generation = e->es_generation;
        stats->fitness_mean = sum / (double)M; stats->fitness_max = mx; stats->fitness_min = mn;
        stats->grad_norm = std::sqrt(gg); stats->theta_norm = std::sqrt(tt);
    }
    return ADC_OK;
}

ADC_EXPORT int adc_engine_es_state_get(adc_engine *e, float *theta_p, float *m_p, float *v_p, int64_t *generation)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = es_ready(e)) return rc;
    ENGINE_GUARD(e);
    const size_t bytes = (size_t)e->pl.P * 4;
    if (theta_p) HIP_TRY(hipMemcpyAsync(theta_p, e->es_theta, bytes, hipMemcpyDeviceToHost, e->stream));
    if (m_p) HIP_TRY(hipMemcpyAsync(m_p, e->es_m, bytes, hipMemcpyDeviceToHost, e->stream));
    if (v_p) HIP_TRY(hipMemcpyAsync(v_p, e->es_v, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (generation) *generation = e->es_generation;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_es_state_set(adc_engine *e, const float *theta_p, const float *m_p, const float *v_p, int64_t generation)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = es_ready(e)) return rc;
    if (!theta_p || !m_p || !v_p) return fail(ADC_EINVAL, "theta, m or v is NULL");
    if (generation < 0 || generation > 0x7FFFFFFFll) return fail(ADC_EINVAL, "generation: 0 to 2^31 - 1");
    ENGINE_GUARD(e);
    const size_t bytes = (size_t)e->pl.P * 4;
    HIP_TRY(hipMemcpyAsync(e->es_theta, theta_p, bytes, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->es_m, m_p, bytes, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->es_v, v_p, bytes, hipMemcpyHostToDevice, e->stream));
    // (the centre's chain-major copy follows theta, so that evaluation without a population sees it)
    hipLaunchKernelGGL(k_params_copy, dim3((unsigned)((e->pl.P + kEsBlock - 1) / kEsBlock)), dim3(kEsBlock), 0, e->stream, e->pl, centre_store(e),
                       e->es_theta, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->es_generation = generation;
    e->es_accumulate = false;
    e->es_days = 0;
    return ADC_OK;
}
