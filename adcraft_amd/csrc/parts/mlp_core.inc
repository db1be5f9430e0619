// mlp_core.inc - what the host files of the learned agent (parts/mlp_api.inc, parts/es_api.inc, parts/rollout_api.inc) and the
// trainers' files after them share: the owned allocations, the agent's view of an env group, the policy kernel's launch, the
// record's slot, a day of the agent, the parameter stores and the flat order against them, the checks several entry points open
// with, the layer upload - and, under a heading of its own at the end, the lifetime chain: who ends when what ends.
// (part of the single translation unit adc_engine.hip)
namespace {
// ---- the owned allocations ---------------------------------------------------------------------------------------------------------
// (dev_alloc of parts/host_api.inc is the engine's own twin of this: its failure text differs, and the texts are part of the contract)
template <typename T>
int mlp_alloc(adc_engine *e, std::vector<void *> &owner, T **p, size_t count)
{
    void *q = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(T), sizeof(T));
    if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); return fail(ADC_ENOMEM, "hipMalloc failed (MLP policy)"); }
    owner.push_back(q);
    if (hipMemsetAsync(q, 0, bytes, e->stream) != hipSuccess) return fail(ADC_EHIP, "hipMemsetAsync failed");
    *p = static_cast<T *>(q);
    return ADC_OK;
}
inline void mlp_free(adc_engine *e, std::vector<void *> &owner)
{
    if (!owner.empty()) (void)hipStreamSynchronize(e->stream);
    for (void *q : owner) (void)hipFree(q);
    owner.clear();
}
// the agent's view of the env group that starts at env e0
inline MlpView mlp_view_from(const adc_engine *e, size_t e0)
{
    MlpView p = e->mp;
    const size_t oa = e0 * (size_t)p.A;
    p.key += e0; p.tick += e0; p.mean += oa; p.ls += oa; p.action += oa; p.logp += e0; p.value += e0;
    if (p.member) p.member += e0;
    if (p.hist) { p.hist += e0 * (size_t)p.D; p.last += e0; p.from += e0; }        // (an env's frames are D = frames * (5K+2) floats)
    return p;
}
// the recurrent policy's view of the env group that starts at env e0 (G = 0: the policy is feed-forward)
inline MlpGruView gru_view_from(const adc_engine *e, size_t e0)
{
    MlpGruView g = e->gv;
    if (g.G) { g.h += e0 * 2u * (size_t)g.G; g.last += e0; g.from += e0; }
    return g;
}
// the term of the flat order that a policy layer is: with a cell the output layer stands behind Wi and Wh
inline int policy_term(const adc_engine *e, int layer) { return e->gv.G && layer >= e->gv.at ? layer + 2 : layer; }
// what a recurrent policy does not go together with (adc_gru.h): ADC_ESTATE with a sentence, the engine as it was
inline int gru_refuses(const adc_engine *e, const char *what)
{
    if (!e->gv.G) return ADC_OK;
    return fail(ADC_ESTATE, std::string(what) + " with a recurrent policy is not supported (adc_engine_mlp_init_recurrent: training it is the evolution strategy's)");
}
// the frames of the policy's input row (1 before adc_engine_mlp_init)
inline int mlp_frames(const adc_engine *e) { return e->mp.frames > 1 ? e->mp.frames : 1; }
void mlp_launch_kernel(const View &v, const MlpView &p, hipStream_t st, int mode, const float *replay_z, float budget_override, float *d_bids,
                       float *d_budget, const MlpRecordSlot &rec, float *value_out, const MlpGruView *gru = nullptr)
{
    // (the recurrent act is a kernel of its own, parts/kernel_mlp_gru.inc; the bootstrap value reads no state and is the kernels' below)
    if (gru && gru->G && mode == 0) {
        const size_t lds = mlp_gru_lds_floats(p.D, p.P, gru->G) * sizeof(float);
        if (p.member) hipLaunchKernelGGL(k_mlp_policy_gru<1>, dim3((unsigned)v.N), dim3(kMlpBlock), lds, st, v, p, *gru, replay_z, budget_override, d_bids, d_budget, rec);
        else hipLaunchKernelGGL(k_mlp_policy_gru<0>, dim3((unsigned)v.N), dim3(kMlpBlock), lds, st, v, p, *gru, replay_z, budget_override, d_bids, d_budget, rec);
        return;
    }
    // (three instantiations: without members the kernel is the single-policy code, untouched by the members' addressing; learners
    // have no pop_stride; the squashed forms are instantiations of their own, and so are the ones with an observation history)
    const dim3 grid((unsigned)v.N), block(kMlpBlock);
    const size_t lds = mlp_lds_floats(p.D, p.P) * sizeof(float);
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, lds, st, v, p, mode, replay_z, budget_override, d_bids, d_budget, rec, value_out); };
    const bool hist = p.hist != nullptr;
    if (p.bd_lo && !(p.member && p.pop_stride != 0)) {          // (the bounded act: the single policy's or the learners'; never a population's)
        if (p.member) hist ? launch(k_mlp_policy<2, false, true, true>) : launch(k_mlp_policy<2, false, false, true>);
        else hist ? launch(k_mlp_policy<0, false, true, true>) : launch(k_mlp_policy<0, false, false, true>);
    } else if (p.member && p.pop_stride == 0 && p.sq_lo) hist ? launch(k_mlp_policy<2, true, true>) : launch(k_mlp_policy<2, true>);
    else if (p.member && p.pop_stride == 0) hist ? launch(k_mlp_policy<2, false, true>) : launch(k_mlp_policy<2>);
    else if (p.member) hist ? launch(k_mlp_policy<1, false, true>) : launch(k_mlp_policy<1>);
    else if (p.sq_lo) hist ? launch(k_mlp_policy<0, true, true>) : launch(k_mlp_policy<0, true>);
    else hist ? launch(k_mlp_policy<0, false, true>) : launch(k_mlp_policy<0>);
}
int mlp_ready(const adc_engine *e)
{
    if (!e->have_mlp) return fail(ADC_ESTATE, "adc_engine_mlp_init has not been called");
    for (int l = 0; l < e->mp.pol.layers; ++l)
        if (!e->mlp_layer_set[0][l]) return fail(ADC_ESTATE, "a policy layer has not been uploaded (adc_engine_mlp_set_layer)");
    if (e->gv.G && !e->gru_set) return fail(ADC_ESTATE, "the cell has not been uploaded (adc_engine_mlp_set_gru)");
    for (int l = 0; l < e->mp.val.layers; ++l)
        if (!e->mlp_layer_set[1][l]) return fail(ADC_ESTATE, "a value layer has not been uploaded (adc_engine_mlp_set_layer)");
    if (e->mlp_cfg.normalize && !e->mlp_norm_set) return fail(ADC_ESTATE, "the normalisation vectors have not been uploaded (adc_engine_mlp_set_norm)");
    if (!e->mp.two_heads && !e->mlp_log_std_set) return fail(ADC_ESTATE, "log_std has not been uploaded (adc_engine_mlp_set_log_std)");
    return ADC_OK;
}
inline bool rollout_room(const adc_engine *e, long long more) { return e->ro_T == 0 || (long long)e->ro_t + more <= (long long)e->ro_T; }
// the record's slot t for the envs from e0 on (all null when `record` is false)
inline MlpRecordSlot rollout_slot(const adc_engine *e, bool record, int t, size_t e0)
{
    MlpRecordSlot r{nullptr, nullptr, nullptr, nullptr, 0};
    if (!record) return r;
    r.raw_obs = (e->tn.obs.count || e->sn.obs.count) ? 1 : 0;
    const size_t n = (size_t)e->v.N, row = (size_t)t * n + e0;
    r.action = e->ro_action + row * (size_t)e->mp.A;
    r.logp = e->ro_logp + row;
    r.value = e->ro_value + row;
    if (e->ro_obs) r.obs = e->ro_obs + row * (size_t)e->mp.D;
    return r;
}
// act on the engine's last observation, group by group inside a chain; `record`: also into slot ro_t of the record
// (the callers have checked mlp_ready)
int mlp_act_chained(adc_engine *e, float budget_override, bool record)
{
    const int t = e->ro_t;
    return launch_chained(e, [&](const View &v, const PolicyView &, hipStream_t st, float *d_bids, float *d_budget) {
        const size_t e0 = (size_t)(d_budget - e->d_budget);       // (the group's first env)
        const MlpGruView g = gru_view_from(e, e0);
        mlp_launch_kernel(v, mlp_view_from(e, e0), st, 0, nullptr, budget_override, d_bids, d_budget, rollout_slot(e, record, t, e0), nullptr, &g);
    });
}
int mlp_record_outcome_chained(adc_engine *e)
{
    const int t = e->ro_t;
    const int rc = launch_chained(e, [&](const View &v, const PolicyView &, hipStream_t st, float *, float *d_budget) {
        const size_t row = (size_t)t * (size_t)e->v.N + (size_t)(d_budget - e->d_budget);
        hipLaunchKernelGGL(k_mlp_record_outcome, dim3((unsigned)((v.N + 255) / 256)), dim3(256), 0, st, v, e->ro_reward + row, e->ro_term + row,
                           e->ro_trunc + row);
    });
    if (!rc) { e->ro_t += 1; e->pg_adv_ready = e->im_adv_ready = false; e->ro_moves = e->env_moves; }
    return rc;
}
// the evolution strategy's side of a stepped day: every env's reward added to its return of the generation
int es_accumulate_chained(adc_engine *e)
{
    const int rc = launch_chained(e, [&](const View &v, const PolicyView &, hipStream_t st, float *, float *d_budget) {
        hipLaunchKernelGGL(k_es_accumulate, dim3((unsigned)((v.N + 255) / 256)), dim3(256), 0, st, v, e->es_return + (size_t)(d_budget - e->d_budget));
    });
    if (!rc) e->es_days += 1;
    return rc;
}
// one day of the learned agent: act (+ the per-step ideal profit when asked for and curves are built), the env's step, the record
int mlp_day(adc_engine *e, float budget_override, bool with_ideal)
{
    const bool record = e->ro_T > 0;
    if (record && !rollout_room(e, 1)) return fail(ADC_EINVAL, "the rollout record is full: adc_engine_rollout_reset before recording another day");
    int rc;
    if (record && e->mp.deterministic) e->ro_deterministic = true;
    // (a day recorded after the envs moved outside the record does not follow the unstored day before it)
    if (record && (e->have_td3 || e->have_td3_pop || e->have_sac || e->have_sac_pop) && e->ro_t > e->td3_stored_t && e->env_moves != e->ro_moves) e->td3_gap = true;
    if ((rc = mlp_act_chained(e, budget_override, record))) return rc;
    if (with_ideal && e->have_curves && (rc = ideal_step_chained(e))) return rc;
    if ((rc = launch_step(e, e->d_bids, e->d_budget, nullptr, /* lazy_join = */ true))) return rc;
    if (record && (rc = mlp_record_outcome_chained(e))) return rc;
    return e->es_accumulate ? es_accumulate_chained(e) : ADC_OK;
}
inline unsigned es_quad_blocks(int P) { return (unsigned)(((P + 3) / 4 + kEsBlock - 1) / kEsBlock); }
ParamStore centre_store(const adc_engine *e)
{
    ParamStore s{};
    for (int l = 0; l < e->mp.pol.layers; ++l) {
        const int t = policy_term(e, l);
        s.W[t] = const_cast<float *>(e->mp.pol.W[l]); s.b[t] = const_cast<float *>(e->mp.pol.b[l]);
    }
    if (e->gv.G) {                      // (the cell's two terms, in front of the output layer)
        const int at = e->gv.at;
        s.W[at] = const_cast<float *>(e->gv.Wi); s.b[at] = const_cast<float *>(e->gv.bi);
        s.W[at + 1] = const_cast<float *>(e->gv.Wh); s.b[at + 1] = const_cast<float *>(e->gv.bh);
    }
    return s;
}
ParamStore member_store(const adc_engine *e, int member)
{
    ParamStore s{};
    float *base = const_cast<float *>(e->mp.pop) + (size_t)member * e->mp.pop_stride;
    for (int l = 0; l < e->pl.layers; ++l) { s.W[l] = base + e->pl.offW[l]; s.b[l] = base + e->pl.offb[l]; }
    return s;
}
// the store's parameters in the flat order, to the host
int params_fetch(adc_engine *e, const ParamStore &s, float *flat)
{
    hipLaunchKernelGGL(k_params_copy, dim3((unsigned)((e->pl.P + kEsBlock - 1) / kEsBlock)), dim3(kEsBlock), 0, e->stream, e->pl, s, e->mlp_flat, 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(flat, e->mlp_flat, (size_t)e->pl.P * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}
inline unsigned pg_blocks(int Q) { return (unsigned)((Q + kPgBlock - 1) / kPgBlock); }
// the flat order of `count` networks' layers, then of a free log_std's A cells (null: none), against their stores: the one walk
// under the learners' centre and members, the single learner's trainer (parts/pg_api.inc) and the off-policy trainers' vectors
PgLayout flat_layout(const MlpNet *nets, int count, const float *log_std = nullptr, int A = 0)
{
    PgLayout lay{};
    int flat = 0, i = 0;
    for (int n = 0; n < count; ++n)
        for (int l = 0; l < nets[n].layers; ++l, ++i) {
            lay.flat0[i] = flat; lay.n_in[i] = nets[n].n_in[l]; lay.n_out[i] = nets[n].n_out[l];
            lay.W[i] = const_cast<float *>(nets[n].W[l]); lay.b[i] = const_cast<float *>(nets[n].b[l]);
            flat += (nets[n].n_in[l] + 1) * nets[n].n_out[l];
        }
    if (log_std) {
        lay.flat0[i] = flat; lay.n_in[i] = 0; lay.n_out[i] = A; lay.W[i] = nullptr; lay.b[i] = const_cast<float *>(log_std);
        flat += A; ++i;
    }
    lay.nterms = i; lay.Q = flat;
    return lay;
}
// ... the policy's own: its layers, its value layers, its log_std unless it is two-headed
PgLayout centre_layout(const adc_engine *e)
{
    const MlpNet nets[2] = {e->mp.pol, e->mp.val};
    return flat_layout(nets, 2, e->mp.two_heads ? nullptr : e->mp.log_std, e->mp.A);
}
// ---- what several entry points open with (mlp_have: only where exactly these two sentences come first, in this order) --------------
int mlp_have(const adc_engine *e)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->have_mlp) return fail(ADC_ESTATE, "adc_engine_mlp_init has not been called");
    return ADC_OK;
}
int population_member_check(const adc_engine *e, int32_t member)
{
    if (e->pop_M == 0) return fail(ADC_ESTATE, "adc_engine_mlp_population has not been called");
    if (member < 0 || member >= e->pop_M) return fail(ADC_EINVAL, "no such member");
    return ADC_OK;
}
int learners_ready(const adc_engine *e, int32_t member)
{
    if (!e->have_mlp) return fail(ADC_ESTATE, "adc_engine_mlp_init has not been called");
    if (e->lrn_M == 0) return fail(ADC_ESTATE, "adc_engine_mlp_learners has not been called");
    if (member < 0 || member >= e->lrn_M) return fail(ADC_EINVAL, "no such member");
    return ADC_OK;
}
// ---- a layer from the host: input-major weights_in_out to adc::mlp_weight_index order, W and b to their stores, the wait -----------------
int mlp_layer_upload(adc_engine *e, float *dW, float *db, int n_in, int n_out, const float *weights_in_out, const float *bias_out)
{
    std::vector<float> w(adc::mlp_weight_count(n_in, n_out), 0.0f);
    for (int j = 0; j < n_in; ++j)
        for (int h = 0; h < n_out; ++h) w[adc::mlp_weight_index(j, h, n_out)] = weights_in_out[(size_t)j * n_out + h];
    HIP_TRY(hipMemcpyAsync(dW, w.data(), w.size() * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(db, bias_out, (size_t)n_out * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}
// ---- the lifetime chain: who ends when what ends ---------------------------------------------------------------------------------------
// These only end things, none allocates, and each calls only what stands above it.  Who calls them (init = adc_engine_mlp_init_frames):
//   norm_set_drop    pg_drop (rn), td3_drop (tn, sn), learners_drop (on, rn), adc_engine_rollout_enable (on), adc_engine_destroy (all
//                    four; parts/host_api.inc), a normaliser's own init and off switch (parts/norm_api.inc)
//   pbt_, kl_, sh_forget   the drops below: a trainer's add-ons only forget, their arrays are the trainer's
//   pg_drop          init, adc_engine_rollout_enable, learners_drop (a population trainer), pg_scratch_alloc (a new trainer; parts/pg_core.inc)
//   td3_drop         init, adc_engine_rollout_enable, learners_drop (a population trainer), the four off-policy inits
//   learners_drop, population_drop   init, adc_engine_mlp_learners, adc_engine_mlp_population (the two kinds of members exclude each other)
// The policy (mlp_allocs) and the record (ro_allocs) end where they are made: init ends all of the above, the policy, then the record.
// a set of normalisers goes - with the policy, the learners, the trainer or the record it was set up for, or with the engine: the
// policy kernel is back to the policy's own vectors, which hold what adc_engine_mlp_set_norm last wrote
void norm_set_drop(adc_engine *e, NormSet &s)
{
    if (s.shared_shift) { e->mp.shift = s.shared_shift; e->mp.scale = s.shared_scale; e->mp.norm_stride = 0; }
    mlp_free(e, s.allocs);
    if (s.obs_part_grown) (void)hipFree(s.obs_part);
    s = NormSet{};
}
// the scheduler of population-based training goes with the population trainer it sits on
void pbt_forget(adc_engine *e, int kind)
{
    if (!e->have_pbt || e->pbt_kind != kind) return;
    e->have_pbt = false;
    e->pbt_round = 0;
    e->pbt_s.clear(); e->pbt_host_fit.clear(); e->pbt_pairs.clear();
    e->pbt_ret = e->pbt_fit = nullptr; e->pbt_dpairs = nullptr;
}
// the KL add-on ends (its arrays stay the trainer's until that goes: a later adc_engine_pg_kl_init finds them)
void kl_forget(adc_engine *e)
{
    e->kl_live = false;
    e->kl_cfg.clear(); e->kl_coef.clear(); e->kl_stats.clear(); e->kl_mem.clear();
}
// the shuffled-minibatches add-on ends (its arrays stay the trainer's until that goes, as the KL add-on's do)
void sh_forget(adc_engine *e)
{
    e->sh_live = e->sh_epoch_ready = false;
    e->sh_mb = 0; e->sh_ns = 0;
    e->sh_cfg.clear(); e->sh_mem.clear(); e->sh_stats.clear(); e->sh_evaluated.clear(); e->sh_last_count.clear();
}
// the policy-gradient trainer goes with the policy and the record it was sized for
void pg_drop(adc_engine *e)
{
    norm_set_drop(e, e->rn);            // (it discounts by this trainer's gamma; the GAE kernels are back to k_pg_gae / k_pg_pop_gae)
    pbt_forget(e, ADC_PBT_PG);
    kl_forget(e);
    e->kl_dmem = nullptr; e->kl_mean_old = e->kl_ls_old = e->kl_pieces = nullptr;      // (its arrays are among pg_allocs)
    sh_forget(e);
    e->sh_dmem = nullptr; e->sh_order = e->sh_rows = nullptr;
    mlp_free(e, e->pg_allocs);
    if (e->pq_host) (void)hipHostFree(e->pq_host);      // (the queued update's pinned twin; its device block was among pg_allocs)
    e->pq_dev = e->pq_host = nullptr; e->pq_bytes = 0;
    e->have_pg = e->have_pg_pop = e->pg_adv_ready = false;
    e->have_im = e->im_adv_ready = false;       // (imitation lives on this trainer's theta and scratch)
    e->pgp_cfg.clear(); e->pgp_steps.clear(); e->pgp_mem.clear(); e->pgp_host_sums.clear();
    e->pgp_dmem = nullptr;
}
// ... and so does the off-policy trainer (its ring holds rows of that policy's input and action widths)
void td3_drop(adc_engine *e)
{
    norm_set_drop(e, e->tn);            // (the record is back to network inputs)
    norm_set_drop(e, e->sn);            // (the SAC learners' normalisers end where their trainer ends)
    e->per_live = false; e->per = PerView{};    // (prioritised replay's arrays are among td3_allocs)
    e->nstep_n = 0; e->nstep_gn = nullptr;      // (so are n-step returns'; a new trainer's rings start without gn)
    pbt_forget(e, ADC_PBT_TD3);
    pbt_forget(e, ADC_PBT_SAC);         // (a SAC population's scheduler: its arrays are among td3_allocs too)
    mlp_free(e, e->td3_allocs);
    e->have_td3 = e->have_td3_pop = e->td3_norm_set = e->td3_gap = e->td3_bounded = false;
    e->have_sac = false;                // (a soft actor-critic learner lives in the same fields, and ends where TD3 ends)
    e->sac_cell = nullptr;
    std::memset(e->td3_critic_set, 0, sizeof(e->td3_critic_set));
    e->td3_updates = e->td3_actor_steps = e->td3_written = 0;
    e->td3_stored_t = 0;
    e->tp_cfg.clear(); e->tp_mem.clear(); e->tp_steps.clear(); e->tp_host_sums.clear(); e->tp_critic_set.clear();
    e->tp_dmem = nullptr; e->tp_dsteps = nullptr;
    e->have_sac_pop = false;            // (a SAC population lives in the TD3 population's fields)
    e->sp_cfg.clear(); e->sp_mem.clear();
    e->sp_dmem = nullptr; e->sp_cells = nullptr;
}
// learners and the population trainer over them go with the policy they belong to (the engine is back to the centre policy)
void learners_drop(adc_engine *e)
{
    norm_set_drop(e, e->on);
    norm_set_drop(e, e->rn);
    kl_forget(e);                       // (as the reward normaliser: a solo trainer survives, its add-ons do not)
    sh_forget(e);
    // (a solo TD3 trainer survives learners and a population, refused while they are active; so do its normalisers, or its raw ring
    //  would be sampled without them afterwards.  A TD3 population's go with it, below)
    if (e->have_pg_pop) pg_drop(e);
    if (e->have_td3_pop || e->have_sac_pop) td3_drop(e);
    mlp_free(e, e->lrn_allocs);
    // (while learners are active a squash is theirs, adc_engine_mlp_learners_set_squash: it goes with them)
    // (... and so are bounds, adc_engine_mlp_learners_set_bounds)
    if (e->lrn_M != 0) {
        e->mp.member = nullptr; e->mp.pop = nullptr; e->mp.pop_stride = 0; e->mp.sq_lo = e->mp.sq_half = nullptr;
        e->mp.bd_lo = e->mp.bd_half = nullptr; e->mp.explore = adc::kMlpGaussian; e->mlp_bd_host.clear();
    }
    e->lrn_M = e->lrn_n = 0;
    e->lrn_block = e->lrn_flat = nullptr; e->lrn_tab = nullptr; e->lrn_stride = 0;
}
// a population and the strategy over it go with the policy they belong to
void population_drop(adc_engine *e)
{
    mlp_free(e, e->pop_allocs);
    mlp_free(e, e->es_allocs);
    e->pop_M = 0;
    e->pop_map.clear();
    e->pop_count.clear();
    e->mp.member = nullptr; e->mp.pop = nullptr; e->mp.pop_stride = 0;
    e->have_es = e->es_accumulate = false;
    e->es_days = 0;
}
}  // namespace
