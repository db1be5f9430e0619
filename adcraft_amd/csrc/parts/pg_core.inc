// pg_core.inc - what the policy-gradient host files (parts/pg_api.inc, parts/pg_kl_api.inc, parts/pg_shuffle_api.inc) share: who
// the members are, the checks an entry point opens with, the sample pass's view, the walk over the gradient's terms, the
// statistics' sums and means, the LDS refusal, the trainer's allocation, a member's state by its flat offset.  A single learner is
// the case of one member: its configuration and its step count are element 0 of pgp_cfg / pgp_steps, and what differs between it
// and a population - the kernels, their arguments, the member table - is a `pop` branch at the launch, never a second function.
// (part of the single translation unit adc_engine.hip)
namespace {
// ---- the members ---------------------------------------------------------------------------------------------------------------
int pg_members(const adc_engine *e) { return e->have_pg_pop ? e->lrn_M : 1; }
int pg_member_envs(const adc_engine *e) { return e->have_pg_pop ? e->lrn_n : e->v.N; }
int pg_Q(const adc_engine *e) { return e->have_pg_pop ? e->lrn_lay.Q : e->pg_lay.Q; }
inline long long pg_chunks(long long n) { return (n + adc::kPgChunk - 1) / adc::kPgChunk; }

// ---- what an entry point checks before it touches the stream; pop: the front end it belongs to ------------------------------------
int pg_ready(const adc_engine *e, bool pop)
{
    if (!(pop ? e->have_pg_pop : e->have_pg))
        return fail(ADC_ESTATE, pop ? "adc_engine_pg_pop_init has not been called (or the policy, the learners or the record were re-initialised since)"
                                    : "adc_engine_pg_init has not been called (or the policy / the record was re-initialised since)");
    return ADC_OK;
}
// what a policy-gradient call needs of the engine's state, checked at init and again at every call
int pg_state_check(const adc_engine *e, bool pop)
{
    if (int rc = mlp_ready(e)) return rc;
    if (int rc = gru_refuses(e, "policy-gradient training")) return rc;
    if (e->mp.bd_lo) return fail(ADC_ESTATE, "policy-gradient training under the bounded act is not supported: it needs a log-probability (adc_engine_mlp_set_bounds(NULL, NULL) first)");
    if (pop) {
        if (e->lrn_M == 0) return fail(ADC_ESTATE, "population training needs learners (adc_engine_mlp_learners)");
    } else {
        if (e->pop_M != 0) return fail(ADC_ESTATE, "policy-gradient training with a population active is not supported (adc_engine_mlp_population(0) first)");
        if (e->lrn_M != 0) return fail(ADC_ESTATE, "learners are active: they train through adc_engine_pg_pop_init (adc_engine_mlp_learners(0) first)");
    }
    if (e->ro_T == 0) return fail(ADC_ESTATE, "policy-gradient training needs a rollout record (adc_engine_rollout_enable)");
    if (!e->ro_obs) return fail(ADC_ESTATE, "policy-gradient training needs the recorded network input (adc_engine_rollout_enable with ADC_ROLLOUT_OBS)");
    return ADC_OK;
}
int pg_record_check(const adc_engine *e)
{
    if (e->ro_t == 0) return fail(ADC_ESTATE, "no day has been recorded (adc_engine_mlp_step / adc_engine_run_days with ADC_POLICY_MLP)");
    if (e->ro_deterministic)
        return fail(ADC_ESTATE, "the record holds days collected with the deterministic policy: their log-probabilities mean nothing "
                                "(adc_engine_mlp_set_deterministic(0), adc_engine_rollout_reset, collect again)");
    if (e->ro_teacher > 0)
        return fail(ADC_ESTATE, "the record holds teacher days: their actions are an expert's, not the policy's (adc_engine_im_update consumes them; "
                                "adc_engine_rollout_reset, collect again)");
    return ADC_OK;
}
// the preamble of the calls that work on the record: the trainer, the engine's state, the record, an update's epochs
int pg_enter(const adc_engine *e, bool pop, int epochs = 1)
{
    int rc;
    if ((rc = pg_ready(e, pop)) || (rc = pg_state_check(e, pop)) || (rc = pg_record_check(e))) return rc;
    if (epochs < 1 || epochs > 65536) return fail(ADC_EINVAL, "epochs: 1 to 65536");
    return ADC_OK;
}
int pg_adv_check(const adc_engine *e, bool pop)
{
    if (!e->pg_adv_ready)
        return fail(ADC_ESTATE, pop ? "adc_engine_pg_pop_advantages has not been called since the last recorded day"
                                    : "adc_engine_pg_advantages has not been called since the last recorded day");
    return ADC_OK;
}
int pg_member_check(const adc_engine *e, int32_t member)
{
    if (member < 0 || member >= pg_members(e)) return fail(ADC_EINVAL, "no such member");
    return ADC_OK;
}
// one trainer at a time owns the policy's weights (the two inits)
int pg_other_trainer_check(const adc_engine *e)
{
    if (e->have_td3 || e->have_td3_pop) return fail(ADC_ESTATE, "an off-policy (TD3) trainer is alive on this engine: one trainer at a time owns the policy's weights");
    if (e->have_sac || e->have_sac_pop) return fail(ADC_ESTATE, "a soft actor-critic trainer is alive on this engine: one trainer at a time owns the policy's weights");
    return ADC_OK;
}
int pg_max_width(const adc::PgShape &sh)
{
    int maxw = 1;
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l < sh.layers[net]; ++l) maxw = std::max(maxw, sh.n_out[net][l]);
    return maxw;
}
// a sample's workgroup keeps its row, its activations and its deltas in LDS: 64 KiB at most.  Which of the two is to blame - the
// keywords, when one frame does not fit either, or the frames (kl: under the KL penalty, in its wording)
int pg_lds_refuse(const adc_engine *e, const adc::PgShape &sh, int maxw, bool kl)
{
    if (pg_lds_floats(sh, maxw, kl) * sizeof(float) <= 64u * 1024u) return ADC_OK;
    const bool keywords = pg_lds_floats(adc::pg_shape_of(e->mlp_cfg, e->v.K), maxw, kl) * sizeof(float) > 64u * 1024u;
    if (kl)
        return fail(ADC_EINVAL, keywords ? "num_keywords too large for the KL penalty (LDS)"
                                         : "frames: the stacked input row is too large for the KL penalty (LDS); fewer frames fit");
    return fail(ADC_EINVAL, keywords ? "num_keywords too large for policy-gradient training (LDS)"
                                     : "frames: the stacked input row is too large for policy-gradient training (LDS); fewer frames fit");
}

// ---- a minibatch --------------------------------------------------------------------------------------------------------------------
// a gathered minibatch (shuffled minibatches: adc_pg_shuffle.h): S samples per member, member m's record rows at rows + m * stride
struct PgGather {
    const uint32_t *rows;
    size_t stride;
    long long S;
};
// (parts/pg_api.inc: the one function of the trainer that the add-ons' update loops call back)
int pg_minibatch_run(adc_engine *e, int n0, int B, adc::PgStatsOut *out_m, const PgGather *g);
// ... the gathered one, with the env range either front end has always handed its sample pass
int pg_gathered_run(adc_engine *e, adc::PgStatsOut *out_m, const PgGather *g) { return pg_minibatch_run(e, 0, e->have_pg_pop ? e->pg_mb : 1, out_m, g); }

// the sample pass's view of the record and the scratch over the envs [n0, n0 + B) (of every member); a single learner's loss
// constants and networks travel in it, a population's are its member and learner tables
PgView pg_view_of(const adc_engine *e, int n0, int B)
{
    PgView p{};
    p.sh = e->pg_shape;
    if (!e->have_pg_pop) {
        const adc_pg_config &c = e->pgp_cfg[0];
        p.loss = adc::PgLoss{c.eps_clip, c.vf_coef, c.ent_coef};
        p.net[0] = e->mp.pol; p.net[1] = e->mp.val;
        p.log_std = e->mp.log_std;
    }
    p.obs = e->ro_obs; p.action = e->ro_action; p.logp = e->ro_logp; p.value = e->ro_value;
    p.adv = e->pg_adv; p.ret = e->pg_ret;
    p.N = e->v.N; p.n0 = n0; p.B = B;
    p.acts = e->pg_acts; p.deltas = e->pg_deltas; p.pieces = e->pg_pieces;
    p.na = adc::pg_acts_floats(p.sh); p.nd = adc::pg_deltas_floats(p.sh); p.maxw = e->pg_maxw;
    return p;
}

// the gradient's terms in the flat order - both networks' layers, then the free log_std: fn(term, its tiles) launches one
template <class Fn>
void pg_terms_walk(const adc::PgShape &sh, const float *obs, const float *acts, int na, Fn fn)
{
    int flat = 0, ao = 0, dof = 0;
    auto term = [&](const float *X, size_t ldx, int n_in, int n_out, int is_obs) {
        fn(PgTerm{X, ldx, n_in, n_out, dof, flat, is_obs}, (unsigned)(((n_in + 1 + kPgTile - 1) / kPgTile) * ((n_out + kPgTile - 1) / kPgTile)));
        flat += (n_in + 1) * n_out;
    };
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l < sh.layers[net]; ++l) {
            const int n_in = adc::pg_n_in(sh, net, l), n_out = sh.n_out[net][l];
            if (l == 0) term(obs, (size_t)sh.D, n_in, n_out, 1);
            else { term(acts + ao, (size_t)na, n_in, n_out, 0); ao += n_in; }
            dof += n_out;
        }
    if (!sh.two_heads) term(nullptr, 0, 0, sh.A, 0);
}

// an epoch's statistics: the minibatches' summed in order, then divided by their count
void pg_stats_add(adc::PgStatsOut &a, const adc::PgStatsOut &o)
{
    a.policy_loss = a.policy_loss + o.policy_loss; a.value_loss = a.value_loss + o.value_loss; a.entropy = a.entropy + o.entropy;
    a.approx_kl = a.approx_kl + o.approx_kl; a.clip_fraction = a.clip_fraction + o.clip_fraction;
    a.grad_norm = a.grad_norm + o.grad_norm; a.explained_variance = a.explained_variance + o.explained_variance;
}
adc::PgStatsOut pg_stats_mean(const adc::PgStatsOut &a, int count)
{
    const double c = (double)count;
    return adc::PgStatsOut{a.policy_loss / c, a.value_loss / c, a.entropy / c, a.approx_kl / c, a.clip_fraction / c, a.grad_norm / c,
                           a.explained_variance / c};
}
void pg_stats_fill(adc_pg_stats *stats, const adc::PgStatsOut &o, int64_t steps, int64_t samples)
{
    stats->steps = steps; stats->samples = samples;
    stats->policy_loss = o.policy_loss; stats->value_loss = o.value_loss; stats->entropy = o.entropy; stats->approx_kl = o.approx_kl;
    stats->clip_fraction = o.clip_fraction; stats->grad_norm = o.grad_norm; stats->explained_variance = o.explained_variance;
}

// the value of the state after the last recorded day, every env's: what GAE bootstraps from
int pg_boot_launch(adc_engine *e)
{
    if (e->mp.val.layers > 0)
        mlp_launch_kernel(e->v, e->mp, e->stream, 1, nullptr, 0.0f, e->d_bids, e->d_budget, MlpRecordSlot{nullptr, nullptr, nullptr, nullptr}, e->mlp_boot);
    else HIP_TRY(hipMemsetAsync(e->mlp_boot, 0, (size_t)e->v.N * 4, e->stream));
    return ADC_OK;
}

// ---- the trainer's arrays -----------------------------------------------------------------------------------------------------------
// A trainer of Ms members with Q parameters each, minibatches of mb envs, `part_stride` doubles of chunk partials a member, replaces
// whatever trainer lived (table: with the population's member table).  The new state is allocated before the old one goes: a
// failure leaves the engine as it was.  cfgs: `count` configurations, one shared by all members or one each
int pg_scratch_alloc(adc_engine *e, const adc::PgShape &sh, int maxw, size_t Ms, size_t Q, int mb, size_t part_stride, bool table, const adc_pg_config *cfgs,
                     int count)
{
    const size_t tn = (size_t)e->ro_T * (size_t)e->v.N, smax = (size_t)e->ro_T * (size_t)mb;
    std::vector<void *> fresh;
    float *theta = nullptr, *m = nullptr, *v = nullptr, *grad = nullptr, *adv = nullptr, *ret = nullptr, *acts = nullptr, *deltas = nullptr, *pieces = nullptr;
    double *part = nullptr, *sums = nullptr, *gpart = nullptr;
    PgMember *dmem = nullptr;
    int rc;
    if ((rc = mlp_alloc(e, fresh, &theta, Ms * Q)) || (rc = mlp_alloc(e, fresh, &m, Ms * Q)) || (rc = mlp_alloc(e, fresh, &v, Ms * Q)) ||
        (rc = mlp_alloc(e, fresh, &grad, Ms * Q)) || (rc = mlp_alloc(e, fresh, &adv, tn)) || (rc = mlp_alloc(e, fresh, &ret, tn)) ||
        (rc = mlp_alloc(e, fresh, &acts, Ms * smax * (size_t)adc::pg_acts_floats(sh))) ||
        (rc = mlp_alloc(e, fresh, &deltas, Ms * smax * (size_t)adc::pg_deltas_floats(sh))) ||
        (rc = mlp_alloc(e, fresh, &pieces, Ms * smax * (size_t)adc::kPgPieces)) || (rc = mlp_alloc(e, fresh, &part, Ms * part_stride)) ||
        (rc = mlp_alloc(e, fresh, &gpart, Ms * (size_t)pg_chunks((long long)smax) * Q)) || (rc = mlp_alloc(e, fresh, &sums, Ms * 16u)) ||
        (table && (rc = mlp_alloc(e, fresh, &dmem, Ms)))) {
        // (rc and its message are mlp_alloc's: ADC_ENOMEM for a refused allocation, ADC_EHIP for a failed memset; no test provokes either)
        mlp_free(e, fresh);
        return rc;
    }
    pg_drop(e);
    e->pg_allocs.swap(fresh);
    e->pg_theta = theta; e->pg_m = m; e->pg_v = v; e->pg_grad = grad; e->pg_adv = adv; e->pg_ret = ret;
    e->pg_acts = acts; e->pg_deltas = deltas; e->pg_pieces = pieces; e->pg_part = part; e->pg_sums = sums; e->pg_gpart = gpart;
    e->pg_mb = mb; e->pg_slots = smax; e->pg_shape = sh; e->pg_maxw = maxw;
    e->pgp_dmem = dmem; e->pgp_part_stride = part_stride;
    e->pgp_cfg.assign(Ms, cfgs[0]);
    if (count > 1) e->pgp_cfg.assign(cfgs, cfgs + Ms);
    e->pgp_steps.assign(Ms, 0);
    return ADC_OK;
}

// ---- a member's state, at its flat offset member * Q (a single learner: member 0) -------------------------------------------------
// the device's layers and log_std follow the member's theta, so that the next act and the next recorded day see it; waits
int pg_params_follow(adc_engine *e, int member)
{
    const int Q = pg_Q(e);
    if (e->have_pg_pop)
        hipLaunchKernelGGL(k_pg_pop_params_copy, dim3(pg_blocks(Q), 1u), dim3(kPgBlock), 0, e->stream, e->lrn_lay, e->lrn_stride, member,
                           e->pg_theta + (size_t)member * (size_t)Q, (size_t)0, 0);
    else
        hipLaunchKernelGGL(k_pg_params_copy, dim3(pg_blocks(Q)), dim3(kPgBlock), 0, e->stream, e->pg_lay, e->pg_theta, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}
int pg_state_get(adc_engine *e, bool pop, int32_t member, float *theta_q, float *m_q, float *v_q, int64_t *steps)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pg_ready(e, pop)) || (rc = pg_member_check(e, member))) return rc;
    ENGINE_GUARD(e);
    const size_t Q = (size_t)pg_Q(e), bytes = Q * 4, at = (size_t)member * Q;
    if (theta_q) HIP_TRY(hipMemcpyAsync(theta_q, e->pg_theta + at, bytes, hipMemcpyDeviceToHost, e->stream));
    if (m_q) HIP_TRY(hipMemcpyAsync(m_q, e->pg_m + at, bytes, hipMemcpyDeviceToHost, e->stream));
    if (v_q) HIP_TRY(hipMemcpyAsync(v_q, e->pg_v + at, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (steps) *steps = e->pgp_steps[(size_t)member];
    return ADC_OK;
}
int pg_state_set(adc_engine *e, bool pop, int32_t member, const float *theta_q, const float *m_q, const float *v_q, int64_t steps)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pg_ready(e, pop)) || (rc = pg_member_check(e, member))) return rc;
    if (!theta_q || !m_q || !v_q) return fail(ADC_EINVAL, "theta, m or v is NULL");
    if (steps < 0 || steps >= 0x7FFFFFFFll) return fail(ADC_EINVAL, "steps: 0 to 2^31 - 2");
    ENGINE_GUARD(e);
    const size_t Q = (size_t)pg_Q(e), bytes = Q * 4, at = (size_t)member * Q;
    HIP_TRY(hipMemcpyAsync(e->pg_theta + at, theta_q, bytes, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->pg_m + at, m_q, bytes, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->pg_v + at, v_q, bytes, hipMemcpyHostToDevice, e->stream));
    if ((rc = pg_params_follow(e, member))) return rc;
    e->pgp_steps[(size_t)member] = steps;
    return ADC_OK;
}
int pg_advantages_fetch(adc_engine *e, bool pop, float *adv_tn, float *ret_tn)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = pg_ready(e, pop)) || (rc = pg_adv_check(e, pop))) return rc;
    ENGINE_GUARD(e);
    const size_t bytes = (size_t)e->ro_t * (size_t)e->v.N * 4;
    if (adv_tn) HIP_TRY(hipMemcpyAsync(adv_tn, e->pg_adv, bytes, hipMemcpyDeviceToHost, e->stream));
    if (ret_tn) HIP_TRY(hipMemcpyAsync(ret_tn, e->pg_ret, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}
}  // namespace
