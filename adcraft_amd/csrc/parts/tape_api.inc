// tape_api.inc - the extern "C" entry points of the tape and of the per-click outcome lists (include/adcraft_engine.h; the kernel is
// k_step_exact of parts/kernel_exact_serial.inc), over parts/host_api.inc: the read-only walk of one env-step, a host tape on the
// device (TapeUpload), the step over a tape, the lists of a step of the engine's own stream and of a step given as a tape.
// (part of the single translation unit adc_engine.hip)

// The paid clicks of one env-step, one by one (see ReplayOut): a read-only second walk of that env-step in the reference's order
// by the serial walker - at the stream position the step had (tape == null), or over the caller's tape.
static int outcomes_walk(adc_engine *e, int32_t env, unsigned int ticks_back, const float *bids_k, float budget, const TapeView *tape, int64_t capacity,
                         int32_t *keyword, int32_t *timestep, double *cost, double *revenue, int64_t *count, int32_t *share_volume_k)
{
    const View &v = e->v;
    if (env < 0 || env >= v.N) return fail(ADC_EINVAL, "env out of range");
    if (!bids_k || !count || capacity < 0 || capacity > (1ll << 28)) return fail(ADC_EINVAL, "bids_k / count is NULL or capacity out of range");
    if (capacity > 0 && (!keyword || !timestep || !cost || !revenue)) return fail(ADC_EINVAL, "output lists are NULL");
    const size_t K = (size_t)v.K, cap = (size_t)capacity;
    const size_t lds = K * (4 * 4 + 3 * 8);
    if (lds > 160 * 1024) return fail(ADC_EINVAL, "num_keywords too large for the walker (LDS)");
    HIP_TRY(hipStreamSynchronize(e->stream));           // the step itself has finished
    unsigned char *d = nullptr;
    const size_t b_rec = (cap ? cap : 1) * sizeof(int4), b_cost = (cap ? cap : 1) * 8, b_bids = K * 4, b_share = K * 4;
    DevTemps tmp(e->stream);
    if (tmp.get(&d, b_rec + b_cost + b_bids + b_share + 16) != hipSuccess) return fail(ADC_ENOMEM, "hipMalloc failed");
    ReplayOut rp{};
    rp.records = reinterpret_cast<int4 *>(d);
    rp.costs = reinterpret_cast<double *>(d + b_rec);
    float *d_bids = reinterpret_cast<float *>(d + b_rec + b_cost);
    rp.share_volume = reinterpret_cast<int *>(d + b_rec + b_cost + b_bids);
    rp.count = reinterpret_cast<int *>(d + b_rec + b_cost + b_bids + b_share);
    rp.bids_env = d_bids;
    rp.budget = budget;
    rp.capacity = (int)capacity;
    rp.env = env;
    rp.ticks_back = ticks_back;
    if (hipMemcpyAsync(d_bids, bids_k, b_bids, hipMemcpyHostToDevice, e->stream) != hipSuccess ||
        hipMemsetAsync(rp.share_volume, 0, b_share + 16, e->stream) != hipSuccess)
        return fail(ADC_EHIP, "upload failed");
    TapeView none{};
#define WALK(MODEL) \
    if (tape) hipLaunchKernelGGL((k_step_exact<MODEL, true>), dim3(1), dim3(kWave), lds, e->stream, v, d_bids, e->d_budget, *tape, 0, rp); \
    else hipLaunchKernelGGL((k_step_exact<MODEL, false>), dim3(1), dim3(kWave), lds, e->stream, v, d_bids, e->d_budget, none, 0, rp)
    if (v.model == ADC_MODEL_IMPLICIT) { WALK(ADC_MODEL_IMPLICIT); }
    else if (v.model == ADC_MODEL_IMPLICIT_GENERAL) { WALK(ADC_MODEL_IMPLICIT_GENERAL); }
    else { WALK(ADC_MODEL_EXPLICIT); }
#undef WALK
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) return fail(ADC_EHIP, "replay kernel failed");
    int n = 0;
    if (hipMemcpy(&n, rp.count, 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(ADC_EHIP, "download failed");
    *count = n;
    const size_t m = std::min<size_t>((size_t)std::max(n, 0), cap);
    if (m) {
        std::vector<int4> rec(m);
        if (hipMemcpy(rec.data(), rp.records, m * sizeof(int4), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(cost, rp.costs, m * 8, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(ADC_EHIP, "download failed");
        for (size_t i = 0; i < m; ++i) {
            keyword[i] = rec[i].x;
            timestep[i] = rec[i].y;
            revenue[i] = rec[i].z < 0 ? -1.0 : (double)rec[i].z / 100.0;
        }
    }
    if (share_volume_k && hipMemcpy(share_volume_k, rp.share_volume, b_share, hipMemcpyDeviceToHost) != hipSuccess) return fail(ADC_EHIP, "download failed");
    tmp.release();
    return ADC_OK;
}

ADC_EXPORT int adc_engine_outcomes_replay(adc_engine *e, int32_t env, int32_t steps_back, const float *bids_k, float budget, int64_t capacity,
                                          int32_t *keyword, int32_t *timestep, double *cost, double *revenue, int64_t *count, int32_t *share_volume_k)
{
    ENGINE_GUARD(e);
    if (!e->have_reset || e->last_step == 0) return fail(ADC_ESTATE, "no step to replay since the reset");
    if (e->last_step == 2) return fail(ADC_ESTATE, "the last step replayed a tape: its variates are the caller's, not the engine's stream (adc_engine_outcomes_replay_tape)");
    if (steps_back < 1 || steps_back > e->stream_steps) return fail(ADC_ESTATE, "steps_back reaches behind the last reset / tape replay");
    if (steps_back > 1 && e->v.drift_on) return fail(ADC_ESTATE, "with drift enabled only the last step can be replayed (the parameters have moved on)");
    if (e->v.drift_on && e->drift_applied)
        return fail(ADC_ESTATE, "the last step's update_keywords() has already been applied to the stored parameters (they were read, or the ideal profit "
                                "evaluated, since the step): its clicks can no longer be regenerated");
    return outcomes_walk(e, env, (unsigned int)steps_back, bids_k, budget, nullptr, capacity, keyword, timestep, cost, revenue, count, share_volume_k);
}

// a host adc_tape on the device (adc_engine_step_replay, adc_engine_outcomes_replay_tape); the copies live as long as the object,
// or until its user, having waited for the stream, releases them
struct TapeUpload {
    adc_engine *e;
    DevTemps tmp;
    TapeView tv{};
    int64_t *d_end = nullptr;
    explicit TapeUpload(adc_engine *engine) : e(engine), tmp(engine->stream) {}
    int up(const void *host, size_t bytes, const void **dev)
    {
        *dev = nullptr;
        if (!host) return ADC_OK;
        void *q = nullptr;
        if (tmp.get(&q, bytes ? bytes : 8) != hipSuccess) return fail(ADC_ENOMEM, "hipMalloc (tape) failed");
        if (bytes && hipMemcpyAsync(q, host, bytes, hipMemcpyHostToDevice, e->stream) != hipSuccess) return fail(ADC_EHIP, "tape upload failed");
        *dev = q;
        return ADC_OK;
    }
    int upload(const adc_tape *tape)
    {
        const size_t N = e->v.N, K = e->v.K, NK = N * K;
        for (size_t i = 0; i < NK; ++i)
            if (tape->volumes[i] < 0 || tape->volumes[i] > adc::kVolumeMax) return fail(ADC_EINVAL, "tape volume out of range [0, 2^20]");
        int rc = ADC_OK;
#define UP(field, type, count) if (!rc) rc = up(tape->field, (size_t)(count) * sizeof(type), (const void **)&tv.field)
        UP(volumes, int32_t, NK);
        UP(bid_cents, int32_t, tape->len_bid);
        UP(x_impressions, int32_t, tape->len_ximp);
        UP(x_cost, double, tape->len_xcost);
        UP(click, uint8_t, tape->len_click);
        UP(conv, uint8_t, tape->len_conv);
        UP(rev_cents, int32_t, tape->len_rev);
        UP(off_bid, int64_t, N); UP(off_ximp, int64_t, N); UP(off_xcost, int64_t, N);
        UP(off_click, int64_t, N); UP(off_conv, int64_t, N); UP(off_rev, int64_t, N);
        if (!rc && tape->drift_uniforms && !e->v.drift_on) rc = fail(ADC_EINVAL, "tape carries drift coefficients but drift is not enabled on this engine");
        UP(drift_uniforms, float, 3 * NK);
#undef UP
        if (!rc && tmp.get(&d_end, 6 * N * 8 + 8) != hipSuccess) rc = fail(ADC_ENOMEM, "hipMalloc (tape cursors) failed");
        if (rc) return rc;
        tv.error = reinterpret_cast<int *>(d_end + 6 * N);
        if (hipMemsetAsync(tv.error, 0, 8, e->stream) != hipSuccess) return fail(ADC_EHIP, "memset failed");
        tv.end_bid = d_end; tv.end_ximp = d_end + N; tv.end_xcost = d_end + 2 * N;
        tv.end_click = d_end + 3 * N; tv.end_conv = d_end + 4 * N; tv.end_rev = d_end + 5 * N;
        tv.len_bid = tape->len_bid; tv.len_ximp = tape->len_ximp; tv.len_xcost = tape->len_xcost;
        tv.len_click = tape->len_click; tv.len_conv = tape->len_conv; tv.len_rev = tape->len_rev;
        return ADC_OK;
    }
    int check_exhausted()
    {
        int tape_error = 0;
        if (hipMemcpy(&tape_error, tv.error, 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(ADC_EHIP, "tape error flag download failed");
        if (tape_error) return fail(ADC_EINVAL, "tape exhausted: the step needed more variates than a tape holds (outputs are invalid)");
        return ADC_OK;
    }
};

ADC_EXPORT int adc_engine_step_replay(adc_engine *e, const float *bids_nk, const float *budget_n, const adc_tape *tape,
                                      adc_step_out *out)
{
    ENGINE_GUARD(e);
    if (!e->have_reset) return fail(ADC_ESTATE, "reset required, need to generate keywords to bid on");
    if (!bids_nk || !budget_n || !tape || !tape->volumes) return fail(ADC_EINVAL, "bids/budget/tape is NULL");
    const size_t N = e->v.N, K = e->v.K, NK = N * K;
    TapeUpload t(e);
    int rc = t.upload(tape);
    if (rc) return rc;
    hipError_t err = hipMemcpyAsync(e->d_bids, bids_nk, NK * 4, hipMemcpyHostToDevice, e->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(e->d_budget, budget_n, N * 4, hipMemcpyHostToDevice, e->stream);
    if (err != hipSuccess) return fail(ADC_EHIP, "action upload failed");
    rc = launch_step(e, e->d_bids, e->d_budget, &t.tv);
    if (!rc) rc = fetch(e, out);
    if (rc) return rc;
    rc = t.check_exhausted();
    if (!rc) {
        int64_t *dst[6] = {tape->end_bid, tape->end_ximp, tape->end_xcost, tape->end_click, tape->end_conv, tape->end_rev};
        for (int i = 0; i < 6 && !rc; ++i)
            if (dst[i] && hipMemcpy(dst[i], t.d_end + i * N, N * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(ADC_EHIP, "cursor download failed");
    }
    t.tmp.release();                // (fetch has waited for the stream)
    return rc;
}

// The same lists for a step given as a TAPE (the reference's recorded variates): env `env` is walked over the caller's tape,
// read-only - no state, output or cursor of the engine is written - with the keyword parameters as they stand.
ADC_EXPORT int adc_engine_outcomes_replay_tape(adc_engine *e, int32_t env, const float *bids_k, float budget, const adc_tape *tape, int64_t capacity,
                                               int32_t *keyword, int32_t *timestep, double *cost, double *revenue, int64_t *count, int32_t *share_volume_k)
{
    ENGINE_GUARD(e);
    if (!e->have_reset) return fail(ADC_ESTATE, "reset required, need to generate keywords to bid on");
    if (!tape || !tape->volumes) return fail(ADC_EINVAL, "tape is NULL");
    TapeUpload t(e);
    int rc = t.upload(tape);
    if (!rc) rc = outcomes_walk(e, env, 0u, bids_k, budget, &t.tv, capacity, keyword, timestep, cost, revenue, count, share_volume_k);
    if (rc) return rc;
    rc = t.check_exhausted();
    t.tmp.release();                // (outcomes_walk has waited for the stream)
    return rc;
}
