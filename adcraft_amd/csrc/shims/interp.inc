// interp.inc (part of adc_shims.cpp) - the interpolation agent's act on the host (adc_interp.h: the code parts/kernel_interp_agent.inc runs)
ADC_EXPORT double adc_interp_key_host(float bid) { return adc::interp_key(bid); }

ADC_EXPORT int adc_interp_act_host(float ave_rpc, int32_t n_rpc, float ave_sctr, int32_t n_sctr, double max_observed, double threshold,
                                   double bid_step, const double *grid, int32_t n_bids, int32_t n_clk, const uint16_t *clk_cent,
                                   const float *clk_ave, int32_t n_cpc, const uint16_t *cpc_cent, const double *cpc_ave, double u,
                                   double *margin_out, double *cost_out, double *bid_out, int32_t *index_out,
                                   double *mass_out)
{
    if (n_bids < 1 || n_bids > adc::kInterpMaxBids || !grid || n_clk < 0 || n_cpc < 0 || n_clk > adc::kInterpCents ||
        n_cpc > n_clk || (n_clk > 0 && (!clk_cent || !clk_ave)) || (n_cpc > 0 && (!cpc_cent || !cpc_ave)) || !bid_out || !index_out)
        return ADC_EINVAL;
    for (int i = 0; i < n_clk; ++i)
        if (clk_cent[i] < 1 || clk_cent[i] > adc::kInterpCents || (i > 0 && clk_cent[i] <= clk_cent[i - 1])) return ADC_EINVAL;
    for (int i = 0; i < n_cpc; ++i)
        if (cpc_cent[i] < 1 || cpc_cent[i] > adc::kInterpCents || (i > 0 && cpc_cent[i] <= cpc_cent[i - 1])) return ADC_EINVAL;
    const adc::InterpSeries<float> clk{clk_cent, clk_ave, 1, n_clk};
    const adc::InterpSeries<double> cpc{cpc_cent, cpc_ave, 1, n_cpc};
    double cpc_right = 0.0;
    for (int i = 0; i < n_cpc; ++i) cpc_right = (i == 0 || cpc_ave[i] > cpc_right) ? cpc_ave[i] : cpc_right;
    const double erpc = adc::interp_erpc(ave_rpc, n_rpc, ave_sctr, n_sctr);
    const double thr = adc::interp_threshold(n_rpc, n_sctr, threshold);
    const int end = adc::interp_end_index(max_observed, bid_step, n_bids);
    auto eval = [&](int j) { return adc::interp_point(clk, cpc, cpc_right, erpc, grid[j]); };
    for (int j = 0; j < n_bids; ++j) {
        const adc::InterpPoint q = eval(j);
        if (margin_out) margin_out[j] = q.margin;
        if (cost_out) cost_out[j] = q.cost;
    }
    const adc::InterpPick pk = adc::interp_pick(eval, thr, end, [&]() { return u; });
    *index_out = pk.index;
    if (mass_out) *mass_out = pk.mass;
    *bid_out = pk.index >= 0 ? grid[pk.index] : 0.01;
    return ADC_OK;
}
