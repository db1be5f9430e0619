// gru_api.inc - the extern "C" entry points of the recurrent policy (include/adcraft_engine.h; the law is csrc/adc_gru.h, the kernel
// parts/kernel_mlp_gru.inc), over parts/mlp_core.inc and the init of parts/mlp_api.inc: the init with a cell, the cell's upload into
// the centre or a member, the state to the host and back, the forget.
// (part of the single translation unit adc_engine.hip)
ADC_EXPORT int adc_engine_mlp_init_recurrent(adc_engine *e, const adc_mlp_config *cfg, const uint64_t *seeds_n, int32_t gru_width)
{
    if (gru_width < 0 || gru_width > adc::kGruMaxWidth) return fail(ADC_EINVAL, "gru_width: 0 (feed-forward) to 256");
    return mlp_init_core(e, cfg, seeds_n, 1, gru_width);
}

ADC_EXPORT int adc_engine_mlp_gru_width(adc_engine *e, int32_t *width)
{
    if (int rc = mlp_have(e)) return rc;
    if (!width) return fail(ADC_EINVAL, "width is NULL");
    *width = e->gv.G;
    return ADC_OK;
}

namespace {
int gru_have(const adc_engine *e)
{
    if (int rc = mlp_have(e)) return rc;
    if (!e->gv.G) return fail(ADC_ESTATE, "the policy is not recurrent (adc_engine_mlp_init_recurrent, gru_width > 0)");
    return ADC_OK;
}
// Wi | bi and Wh | bh, input-major, into the two terms of a store
int gru_upload(adc_engine *e, const ParamStore &s, const float *wi_in_3g, const float *bi_3g, const float *wh_g_3g, const float *bh_3g)
{
    const int at = e->gv.at, G3 = 3 * e->gv.G;
    if (int rc = mlp_layer_upload(e, s.W[at], s.b[at], e->gv.n_in, G3, wi_in_3g, bi_3g)) return rc;
    return mlp_layer_upload(e, s.W[at + 1], s.b[at + 1], e->gv.G, G3, wh_g_3g, bh_3g);
}
}  // namespace

ADC_EXPORT int adc_engine_mlp_set_gru(adc_engine *e, const float *wi_in_3g, const float *bi_3g, const float *wh_g_3g, const float *bh_3g)
{
    if (int rc = gru_have(e)) return rc;
    if (!wi_in_3g || !bi_3g || !wh_g_3g || !bh_3g) return fail(ADC_EINVAL, "a weight matrix or a bias of the cell is NULL");
    ENGINE_GUARD(e);
    if (int rc = gru_upload(e, centre_store(e), wi_in_3g, bi_3g, wh_g_3g, bh_3g)) return rc;
    e->gru_set = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_mlp_set_member_gru(adc_engine *e, int32_t member, const float *wi_in_3g, const float *bi_3g, const float *wh_g_3g,
                                             const float *bh_3g)
{
    if (int rc = gru_have(e)) return rc;
    if (int rc = population_member_check(e, member)) return rc;
    if (!wi_in_3g || !bi_3g || !wh_g_3g || !bh_3g) return fail(ADC_EINVAL, "a weight matrix or a bias of the cell is NULL");
    ENGINE_GUARD(e);
    return gru_upload(e, member_store(e, member), wi_in_3g, bi_3g, wh_g_3g, bh_3g);
}

// the state to the host and back (any pointer may be NULL): h[N][2][G], last[N], from[N]; a run resumed from them continues bit for bit
ADC_EXPORT int adc_engine_mlp_hidden_get(adc_engine *e, float *h_n2g, int32_t *last_n, int32_t *from_n)
{
    if (int rc = gru_have(e)) return rc;
    ENGINE_GUARD(e);
    const size_t n = (size_t)e->v.N;
    if (h_n2g) HIP_TRY(hipMemcpyAsync(h_n2g, e->gv.h, n * 2u * (size_t)e->gv.G * 4, hipMemcpyDeviceToHost, e->stream));
    if (last_n) HIP_TRY(hipMemcpyAsync(last_n, e->gv.last, n * 4, hipMemcpyDeviceToHost, e->stream));
    if (from_n) HIP_TRY(hipMemcpyAsync(from_n, e->gv.from, n * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_mlp_hidden_set(adc_engine *e, const float *h_n2g, const int32_t *last_n, const int32_t *from_n)
{
    if (int rc = gru_have(e)) return rc;
    const size_t n = (size_t)e->v.N;
    for (size_t i = 0; i < n; ++i)
        if ((last_n && last_n[i] < adc::kMlpHistNone) || (from_n && from_n[i] < 0)) return fail(ADC_EINVAL, "hidden state: last >= -2 and from >= 0");
    ENGINE_GUARD(e);
    if (h_n2g) HIP_TRY(hipMemcpyAsync(e->gv.h, h_n2g, n * 2u * (size_t)e->gv.G * 4, hipMemcpyHostToDevice, e->stream));
    if (last_n) HIP_TRY(hipMemcpyAsync(e->gv.last, last_n, n * 4, hipMemcpyHostToDevice, e->stream));
    if (from_n) HIP_TRY(hipMemcpyAsync(e->gv.from, from_n, n * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

// every env's next act starts from zeros (what adc_engine_es_perturb does too: the states were computed under other weights)
ADC_EXPORT int adc_engine_mlp_hidden_forget(adc_engine *e)
{
    if (int rc = gru_have(e)) return rc;
    ENGINE_GUARD(e);
    hipLaunchKernelGGL(k_mlp_hist_forget, dim3((unsigned)((e->v.N + 255) / 256)), dim3(256), 0, e->stream, e->v.N, nullptr, e->gv.last);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}
