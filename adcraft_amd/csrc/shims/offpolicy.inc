// offpolicy.inc (part of adc_shims.cpp) - what the TD3 and the SAC host twins share (shims/td3.inc, shims/sac.inc): the clauses their configuration checks
// have in common, one network's gradient terms, the twin critics' gradient.  The device side's counterpart is parts/offpolicy_core.inc.
namespace {
// The clauses adc_td3_config_check and adc_sac_config_check share, as two runs: each check holds its own clauses between them, and
// reports the first clause that fails in its own order.  A run returns that clause's sentence, or null.
template <class Config>
const char *offpolicy_discount_clause(const Config &c)
{
    if (!(c.gamma >= 0.0f && c.gamma <= 1.0f)) return "gamma: 0 to 1";
    if (!(c.tau > 0.0f && c.tau <= 1.0f)) return "tau: above 0, at most 1";
    return nullptr;
}
// reward_scale, the ring, the critics' shape, the steps (the optimiser's constants are ADC_TD3_* in both configurations)
template <class Config>
const char *offpolicy_training_clause(const Config &c)
{
    const float inf = __builtin_inff();
    if (!(c.reward_scale != 0.0f && c.reward_scale > -inf && c.reward_scale < inf)) return "reward_scale must be finite and not 0";
    if (c.batch_size < 1 || c.batch_size > (1 << 20)) return "batch_size: 1 to 2^20";
    if (c.capacity < 1 || c.capacity > (1 << 30)) return "capacity: 1 to 2^30";
    if (c.n_critic_layers < 1 || c.n_critic_layers > adc::kMlpMaxLayers) return "n_critic_layers: 1 to 4";
    if (c.critic_widths[c.n_critic_layers - 1] != 1) return "the last critic layer has one output";
    if (!(c.actor_lr >= 0.0f && c.actor_lr < inf)) return "actor_lr >= 0";
    if (!(c.critic_lr >= 0.0f && c.critic_lr < inf)) return "critic_lr >= 0";
    if (c.optimiser != ADC_TD3_ADAM && c.optimiser != ADC_TD3_SGD) return "unknown optimiser";
    if (c.optimiser == ADC_TD3_ADAM && (!(c.beta1 >= 0.0f && c.beta1 < 1.0f) || !(c.beta2 >= 0.0f && c.beta2 < 1.0f))) return "Adam: 0 <= beta1, beta2 < 1";
    if (c.optimiser == ADC_TD3_ADAM && !(c.eps > 0.0f)) return "Adam: eps > 0";
    if (!(c.max_grad_norm >= 0.0f && c.max_grad_norm < inf)) return "max_grad_norm >= 0 (0: off)";
    for (int l = 0; l + 1 < c.n_critic_layers; ++l)
        if (c.critic_widths[l] < 1 || c.critic_widths[l] > adc::kMlpMaxWidth) return "hidden critic widths: 1 to 256";
    return nullptr;
}
// what the two families' population checks (pg.inc's pop_config_clause) ask to be equal in a member c and the first, c0: the ring,
// the family's own field - own_equal, own_sentence - and the critics' shape, in that order
template <class Config>
const char *offpolicy_unequal(const Config &c, const Config &c0, bool own_equal, const char *own_sentence)
{
    const char *shape = "n_critic_layers / critic_widths must be equal in all members' configurations (the critics' shape is shared)";
    if (c.batch_size != c0.batch_size) return "batch_size must be equal in all members' configurations (their updates run in the same launches)";
    if (c.capacity != c0.capacity) return "capacity must be equal in all members' configurations (their rings move together)";
    if (!own_equal) return own_sentence;
    if (c.n_critic_layers != c0.n_critic_layers) return shape;
    for (int l = 0; l < c.n_critic_layers; ++l)
        if (c.critic_widths[l] != c0.critic_widths[l]) return shape;
    return nullptr;
}

// one network's gradient terms in the flat order: g[flat0 ...] = float32(csum over the batch / count)
void td3_net_grad_host(const adc::Td3Net &net, int64_t count, const float *X0, size_t ldx0, const float *ys, size_t ny, size_t y_off, const float *deltas,
                       size_t nd, size_t d_off, float *g)
{
    size_t q = 0, lo = 0;
    for (int l = 0; l < net.layers; ++l) {
        const int n_in = adc::td3_n_in(net, l), n_out = net.n_out[l];
        const float *X = l == 0 ? X0 : ys + y_off + lo - (size_t)n_in;
        const size_t ldx = l == 0 ? ldx0 : ny;
        for (int j = 0; j <= n_in; ++j)
            for (int h = 0; h < n_out; ++h) {
                const double total = adc::pg_csum(count, [&](double part, int64_t s) {
                    return adc::pg_chain_mac(part, j < n_in ? X[(size_t)s * ldx + (size_t)j] : 1.0f, deltas[(size_t)s * nd + d_off + lo + (size_t)h]);
                });
                g[q++] = adc::pg_grad_finish(total, count);
            }
        lo += (size_t)n_out;
    }
}

// the smaller of the twin critics psi_q [2][Qc] on the row (x, a); yq: scratch of td3_outs(sh.q)
float offpolicy_min_q_host(const adc::Td3Shape &sh, const float *psi_q, const float *row, std::vector<float> &yq)
{
    float q[2];
    for (int i = 0; i < 2; ++i) {
        adc::td3_forward_host(sh.q, sh.activation, psi_q + (size_t)i * (size_t)adc::td3_params(sh.q), row, yq.data());
        q[i] = yq[(size_t)adc::td3_hidden(sh.q)];
    }
    return adc::td3_min(q[0], q[1]);
}

// the twin critics' gradient on a batch: rows x_bd with the action columns action_of(s, a) writes as the critics read them
template <class ActionOf>
void offpolicy_critic_grad_host(const adc::Td3Shape &sh, const float *psi_q, int32_t count, const float *x_bd, const float *y_b, float *grad_q, double *sums6,
                                ActionOf action_of)
{
    const size_t S = (size_t)count, D = (size_t)sh.D, A = (size_t)sh.A, DA = D + A, Qc = (size_t)adc::td3_params(sh.q), no = (size_t)adc::td3_outs(sh.q),
                 nh = (size_t)adc::td3_hidden(sh.q);
    std::vector<float> xin(S * DA), ys(S * 2 * no), deltas(S * 2 * no), pieces(S * adc::kTd3Pieces, 0.0f);
    for (size_t s = 0; s < S; ++s) {
        float *row = xin.data() + s * DA;
        std::copy(x_bd + s * D, x_bd + (s + 1) * D, row);
        for (size_t a = 0; a < A; ++a) row[D + a] = action_of(s, a);
        for (size_t i = 0; i < 2; ++i) {
            float *y = ys.data() + s * 2 * no + i * no, *d = deltas.data() + s * 2 * no + i * no;
            adc::td3_forward_host(sh.q, sh.activation, psi_q + i * Qc, row, y);
            float loss;
            d[nh] = adc::td3_critic_delta(y[nh], y_b[s], loss);
            pieces[s * adc::kTd3Pieces + adc::kTd3Loss1 + i] = loss;
            pieces[s * adc::kTd3Pieces + adc::kTd3Q1 + i] = y[nh];
            adc::td3_backward_host(sh.q, sh.activation, psi_q + i * Qc, y, d);
        }
        pieces[s * adc::kTd3Pieces + adc::kTd3Y] = y_b[s];
    }
    for (size_t i = 0; i < 2; ++i)
        td3_net_grad_host(sh.q, count, xin.data(), DA, ys.data(), 2 * no, i * no, deltas.data(), 2 * no, i * no, grad_q + i * Qc);
    if (sums6) {
        for (int c = 0; c < 5; ++c) sums6[c] = adc::pg_csum(count, [&](double part, int64_t s) { return part + (double)pieces[(size_t)s * adc::kTd3Pieces + (size_t)c]; });
        sums6[5] = adc::pg_csum((int64_t)(2 * Qc), [&](double part, int64_t p) { return adc::pg_chain_mac(part, grad_q[p], grad_q[p]); });
    }
}
}  // namespace
