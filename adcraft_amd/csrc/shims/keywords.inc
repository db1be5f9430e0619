// keywords.inc (part of adc_shims.cpp) - an EXPLICIT keyword on the host: its sample and its cached bid curve (adc_law.h)
// adcraft/gymnasium_kw_utils.py:113-156 (sample_random_keywords), one keyword: what k_generate_explicit_keywords writes
ADC_EXPORT int adc_sample_random_keyword(uint64_t key, uint32_t keyword, uint32_t serial, float *out8)
{
    if (!out8) return ADC_EINVAL;
    adc::generate_explicit_keyword(key, keyword, serial, out8);
    return ADC_OK;
}

// the host twin of an EXPLICIT keyword's cached bid curve (k_explicit_curves): the same n draws of the ST_METRIC stream, sorted,
// and the same adc::explicit_curve_point on their two middle normals.  cpc is bit-identical to the device's; ir uses the host's exp
// (the device's is ocml's).  z_mid2_out (nullable) receives z_lo, z_hi.
ADC_EXPORT int adc_explicit_curve_host(uint64_t key, uint32_t tick, int32_t keyword, int32_t n_samples, float impression_thresh, float a,
                                       float b, const double *bid_grid, int32_t n_bids, double *ir_out, double *cpc_out, double *z_mid2_out)
{
    if (n_samples <= 0 || n_samples > (1 << 20) || keyword < 0 || n_bids < 0 || (n_bids > 0 && (!bid_grid || !ir_out || !cpc_out)))
        return ADC_EINVAL;
    std::vector<float> z((size_t)n_samples);
    for (int32_t i = 0; i < n_samples; i += 4) {
        const adc::U4 w = adc::draw(key, (uint32_t)(i / 4), adc::ST_METRIC, (uint32_t)keyword, tick);
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
        for (int j = 0; j < 4 && i + j < n_samples; ++j) z[(size_t)(i + j)] = adc::normal_from_word(ws[j]);
    }
    std::sort(z.begin(), z.end());
    const float z_lo = z[(size_t)((n_samples - 1) / 2)], z_hi = z[(size_t)(n_samples / 2)];
    if (z_mid2_out) { z_mid2_out[0] = z_lo; z_mid2_out[1] = z_hi; }
    for (int32_t i = 0; i < n_bids; ++i) {
        double mu, sigma;
        adc::explicit_cost_law(bid_grid[i], mu, sigma);
        const adc::CurvePoint q = adc::explicit_curve_point(impression_thresh, a, b, z_lo, z_hi, bid_grid[i], mu, sigma);
        ir_out[i] = q.ir;
        cpc_out[i] = q.cpc;
    }
    return ADC_OK;
}
