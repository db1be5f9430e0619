// host_api.inc - the engine's core on the host (include/adcraft_engine.h): the engine object; the env groups, their streams and views;
// owned allocations (dev_alloc) and the holder of a call's temporaries (DevTemps); the profile flush and the volume hint; the step's
// plan, launch and fetch, launch_chained; create and destroy; the entry guards; the entry points of the step itself.  What sets or
// reads the envs is parts/env_api.inc, the tape parts/tape_api.inc, metrics and curves parts/curves_api.inc, the two hand-written
// agents parts/agent_api.inc, the engine-less self-tests parts/selftest_api.inc: all of them are written over this file.
// (part of the single translation unit adc_engine.hip; see that file for the overview)
// a set of running normalisers fed from the rollout record (parts/kernel_norm.inc, parts/norm_api.inc): an observation part, a
// reward part, or both; a part that does not live has a null count
struct NormSet {
    bool live = false;
    int M = 0;                          // normalisers: 1 (shared) or the learners' count (per_member)
    int t0 = 0;                         // the record's days [0, t0) have been consumed
    ObsNormView obs{};                  // count, mean, M2 and the vectors the policy kernel reads ([M][D] each)
    const float *shared_shift = nullptr, *shared_scale = nullptr;   // per-member vectors are in force: the policy's own [D] vectors
    double *obs_part = nullptr;         // [M][chunks][2][D] chunk partials
    size_t obs_part_grown = 0;          // doubles of an obs_part grown on demand, which is then not one of `allocs`
    RewNormView rew{};                  // count, mean, M2, the multiplier ([M] each); the envs' carry [N]
    double *g = nullptr;                // [M][S] the discounted returns of an update, in the law's sample order (at most ro_T x N)
    double *rew_part = nullptr;         // [M][chunks][2] chunk partials
    int32_t *src = nullptr;             // [M] the copy's donors
    std::vector<void *> allocs;
};

struct adc_engine {
    adc_config cfg;
    View v;
    hipStream_t stream = nullptr;
    float *d_bids = nullptr, *d_budget = nullptr;
    // small engines (a single env, a few envs): outputs and actions are each ONE device block with a page-locked host
    // mirror, so a host step is one copy each way instead of twelve (each small copy costs ~5 us of latency)
    unsigned char *d_out_block = nullptr, *h_out_block = nullptr;
    size_t out_block_bytes = 0, out_off[10] = {0};
    float *h_act_block = nullptr;        // [NK bids | N budgets], mirrors d_bids (d_budget follows it in the same block)
    std::vector<void *> allocs;
    bool have_reset = false;
    int last_step = 0;                  // 0: none since the reset, 1: a step on the engine's own stream, 2: a tape replay
    int *h_binding = nullptr;           // page-locked word the row kernel sets once a budget binds (View::binding_flag)
    size_t rest_table_count = 0;        // View::rest_table entries to allocate once a budget binds (0: k_step_rest_of_day walks its marks itself)
    size_t click_rec_count = 0;         // View::click_rec entries to allocate once an env asks for lists (0: path off)
    bool in_capture = false;            // inside adc_engine_run_days' stream capture (no allocation there)
    bool h_binding_off = false;         // the rest-of-day table could not be allocated: that path stays off (plan_step)
    bool fail_lazy_alloc = false;       // ADCRAFT_FAIL_LAZY_ALLOC=1 (tests): the two lazy allocations below behave as if hipMalloc had failed
    // env groups (launch_step): streams and events of the groups, the lists' counters of the engine's own view and of every group's
    hipStream_t gstream[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[4] = {nullptr, nullptr, nullptr, nullptr};
    int *d_counters = nullptr;          // [1 + kMaxGroups][kCounterInts]
    int last_groups = 1;                // grouping of the last IMPLICIT step
    bool api_since_step = true;         // anything but adc_engine_step_device (with the engine's own action buffers) was called since the last step
    bool needs_fork = true;             // something may have been enqueued on the engine's stream since the groups last waited for it
    bool groups_pending = false;        // env groups have work in flight that the engine's stream has not been made to wait for yet (join_groups)
    bool stream_exposed = false;        // adc_engine_stream has handed the stream out: the caller may enqueue on it at any time, so the groups wait for it every step
    int group_streams = 0;              // streams in gstream[] (pick_group_streams: one per hardware queue it found, at most four)
    bool no_group_streams = false;      // creating the groups' streams failed once: one group from then on
    int groups_override = 0;            // adc_engine_set_env_groups / ADCRAFT_STREAM_GROUPS at creation (0 = choose; 1..4)
    struct StepPlan { bool lists, rest, direct; } capture_plan{false, false, false};      // what adc_engine_run_days sampled before it began to capture
    int *h_direct = nullptr;            // page-locked word k_rest_walk sets once an env earns hint 6 (View::direct_flag)
    int *h_listing = nullptr;           // page-locked word the kernels set once an env lists its clicked wins (View::listing_flag)
    const char *step_kernel = "";       // the first-pass kernel of the last step (adc_engine_step_kernel_name)
    long long stream_steps = 0;         // consecutive steps on the engine's own stream since the last reset / tape replay / change of parameters or stream position
    bool drift_applied = false;         // with drift on: the last step's pending update_keywords() has already been written into the
                                        // parameter planes (k_materialize_drift), so a replay of that step would read moved parameters
    bool profiling = false;
    int profile_every = 1;                      // bracket every n-th step with events (1 = every step); recording costs ~16 us a step
    unsigned profile_tick = 0;
    long long event_records = 0;        // hipEventRecord calls issued by launch_step since the engine was created
    std::vector<hipEvent_t> ev;          // [kProfileRing][kProfileMarks]
    int ev_used = 0;
    double prof_ms[3] = {0.0, 0.0, 0.0};   // fast pass | exact pass + tail | metric accumulate
    int64_t prof_launches = 0;
    size_t flat_obs_bytes = 0;
    uint32_t step_serial = 0;
    int num_cus = 256;
    int rows_per_cu = 0;
    float mean_volume_hint = -1.0f;     // mean of the vol_mean plane (< 0: unknown); a scheduling hint only, results never depend on it
    bool volume_hint_dirty = true;      // keyword parameters changed since the hint was taken
    double *d_hint_sum = nullptr;
    uint32_t *d_drift_bits = nullptr;   // [N][ceil(K/32)] adc_engine_set_drift_mask's selection, allocated at its first non-null call (View::drift_bits)
    float *d_drift_rate = nullptr;      // [N][3] adc_engine_set_env_drift's magnitudes, allocated at its first non-null call (View::drift_rate)
    unsigned short *d_counts_u16 = nullptr;     // [3][N*K] compact counts (adc_step_out.counts_u16), allocated on first use
    int *d_counts_overflow = nullptr;
    adc_step_out checked_out = {};              // outputs_device_addressable's memo
    bool checked_out_ok = false;
    int fast_tile_kw = 0;                       // ADCRAFT_FAST_TILE_KW: keywords per workgroup of the fast pass (16..256, a power of two)
    int fast_tiles_per_wg = 0;          // 0 = choose from the hint; ADCRAFT_FAST_TILES_PER_WG overrides (experiments)
    int fast_variant = 0;               // 0 = choose from the hint; 1 = interval variant, 2 = sparse variant (ADCRAFT_FAST_VARIANT, experiments)
    float *d_flat_obs = nullptr;
    float *d_flat_actions = nullptr;
    PolicyView pol{};                   // baseline policies + per-step ideal (allocated on first use)
    bool have_agent = false, have_curves = false, have_ideal = false;
    InterpView ip{};                    // the interpolation agent (adc_engine_interp_init; allocated there)
    bool have_interp = false;
    long long interp_updates = 0;       // updates since adc_engine_interp_init: each may add one point per keyword and list
    MlpView mp{};                       // the MLP policy (adc_engine_mlp_init; allocated there)
    bool have_mlp = false;
    adc_mlp_config mlp_cfg{};
    bool mlp_layer_set[2][4] = {{false, false, false, false}, {false, false, false, false}};      // [network][layer] uploaded since init
    bool mlp_norm_set = false, mlp_log_std_set = false;
    float *mlp_boot = nullptr;          // [N] adc_engine_mlp_bootstrap_value's device result
    float *mlp_sq = nullptr;            // [2][A] the squash's lo and half (adc_engine_mlp_set_squash); mp.sq_lo names it while squash is on
    float *mlp_bd = nullptr;            // [3][A] the bounded act's lo, half and 1 / half (adc_engine_mlp_set_bounds); mp.bd_lo names it while it is on
    std::vector<float> mlp_bd_host;     // [2][A] the lo and hi they were formed from (empty: off)
    bool td3_bounded = false;           // adc_engine_td3_set_bounded / adc_engine_td3_pop_set_bounded: the learners' law is the bounded one
    std::vector<void *> mlp_allocs;     // weights, vectors and last-act arrays (re-allocated by every adc_engine_mlp_init)
    MlpGruView gv{};                    // the recurrent policy's cell and state (adc_engine_mlp_init_recurrent; gv.G = 0: feed-forward); among mlp_allocs
    bool gru_set = false;               // the cell uploaded since init (adc_engine_mlp_set_gru)
    // a population of policies (adc_engine_mlp_population) and the evolution strategy over it (adc_engine_es_init; parts/kernel_es.inc)
    ParamLayout pl{};                   // the flat parameter order of the policy network (set by adc_engine_mlp_init)
    float *mlp_flat = nullptr;          // [P] staging of one flat parameter vector
    int pop_M = 0;
    std::vector<int32_t> pop_map;       // [N] env -> member (host copy)
    std::vector<int32_t> pop_count;     // [M] envs per member
    std::vector<void *> pop_allocs;     // the members' layers and the device map (freed by mlp_init and by a new population)
    bool have_es = false, es_accumulate = false;
    adc_es_config es_cfg{};
    uint64_t es_key = 0;
    int64_t es_generation = 0;
    long long es_days = 0;              // days stepped since the last adc_engine_es_perturb
    float *es_theta = nullptr, *es_m = nullptr, *es_v = nullptr, *es_grad = nullptr;     // [P]
    double *es_du = nullptr, *es_return = nullptr;                                        // [M / 2], [N]
    std::vector<void *> es_allocs;
    // learners (adc_engine_mlp_learners): every member's own policy layers, value layers and log_std in one block, a member's
    // part lrn_stride floats long; lrn_lay is member 0's stores against the trainer's flat order theta[Q]
    int lrn_M = 0, lrn_n = 0;           // members; envs of a member
    float *lrn_block = nullptr, *lrn_flat = nullptr;    // [M][lrn_stride]; [Q] staging of one flat parameter vector
    size_t lrn_stride = 0;
    MlpLearner *lrn_tab = nullptr;      // [M] on the device (MlpView::learners)
    PgLayout lrn_lay{};
    std::vector<void *> lrn_allocs;
    // the rollout record (adc_engine_rollout_enable): [T][N][...] arrays, ro_t days recorded so far
    int ro_T = 0, ro_t = 0, ro_fields = 0;
    float *ro_action = nullptr, *ro_logp = nullptr, *ro_value = nullptr, *ro_reward = nullptr, *ro_obs = nullptr;
    uint8_t *ro_term = nullptr, *ro_trunc = nullptr;
    std::vector<void *> ro_allocs;
    bool ro_deterministic = false;      // a recorded day was collected with the deterministic policy: its log-probabilities mean nothing
    // teacher days (adc_engine_teach_days; parts/imitation_api.inc): how many of the record's days an expert acted on, and where the
    // learner's discarded bids and budgets of such a day go ([N][K], then [N]; allocated at the first teacher day)
    int ro_teacher = 0;
    float *teach_act = nullptr;
    std::vector<void *> teach_allocs;
    // DAgger days (adc_engine_dagger_days; the law is adc_dagger.h): how many of the record's teacher days the beta-mixture drove, and
    // one byte per (day, env) of the record - 1: the teacher's action was consumed ([ro_T][N], the record's allocation, made at the
    // first DAgger day of a record; dg_day[t] says which of the record's days wrote their row)
    int ro_dagger = 0;
    uint8_t *dg_mask = nullptr;
    std::vector<uint8_t> dg_day;        // [ro_T] 1: day t of the record is a DAgger day
    // imitation learning over the live single-learner trainer (adc_engine_im_init; parts/kernel_imitation.inc, parts/imitation_api.inc;
    // the law is adc_imitation.h): the moving scale ma, how often it was updated, the scale c of the last advantages call
    bool have_im = false, im_adv_ready = false;
    adc_im_config im_cfg{};
    double im_ma = 0.0;
    int64_t im_calls = 0;
    float im_c = 0.0f;
    // policy-gradient training over the record (adc_engine_pg_init; parts/kernel_pg.inc, parts/pg_core.inc, parts/pg_api.inc)
    bool have_pg = false, pg_adv_ready = false;
    int pg_mb = 0;                      // envs of a minibatch (the scratch's capacity)
    size_t pg_slots = 0;                // samples of a minibatch the scratch holds per member: T * pg_mb, more under shuffled minibatches
    adc::PgShape pg_shape{};
    PgLayout pg_lay{};
    int pg_maxw = 0;
    float *pg_theta = nullptr, *pg_m = nullptr, *pg_v = nullptr, *pg_grad = nullptr;    // [Q]
    float *pg_adv = nullptr, *pg_ret = nullptr;                                          // [T][N]
    float *pg_acts = nullptr, *pg_deltas = nullptr, *pg_pieces = nullptr;                // [T * minibatch envs][...]
    double *pg_part = nullptr, *pg_sums = nullptr;                                       // chunk partials; the law's ten sums
    double *pg_gpart = nullptr;                                                          // [chunks][Q] the weight gradient's partials
    std::vector<void *> pg_allocs;
    // the members' configurations and optimiser steps taken (a single learner is member 0: parts/pg_core.inc)
    std::vector<adc_pg_config> pgp_cfg;         // [M]
    std::vector<int64_t> pgp_steps;             // [M]
    // ... and of a learner population (adc_engine_pg_pop_init; it shares the scratch fields above, sized for all members at once:
    // pg_theta / pg_m / pg_v / pg_grad are [M][Q], pg_acts / pg_deltas / pg_pieces [M][T * minibatch envs][...], pg_sums [M][16])
    bool have_pg_pop = false;
    std::vector<PgMember> pgp_mem;              // [M] the host's copy of pgp_dmem
    std::vector<double> pgp_host_sums;          // [M][16]
    PgMember *pgp_dmem = nullptr;
    size_t pgp_part_stride = 0;                 // doubles of chunk partials per member
    // the KL penalty / value-loss clip add-on of the live PPO / A2C trainer (adc_engine_pg_kl_init; parts/kernel_pg_kl.inc,
    // parts/pg_kl_api.inc; the law is adc_pg_kl.h).  Its device arrays are the trainer's allocations (pg_allocs): they go with it
    bool kl_live = false;
    std::vector<adc_pg_kl_config> kl_cfg;       // [members] (1 for a single learner)
    std::vector<float> kl_coef;                 // [members] the coefficients: the add-on's whole state
    std::vector<adc_pg_kl_stats> kl_stats;      // [members] of the last minibatch / update
    std::vector<PgKlMember> kl_mem;             // [members] the host's copy of kl_dmem (a population's)
    PgKlMember *kl_dmem = nullptr;
    float *kl_mean_old = nullptr, *kl_ls_old = nullptr;     // the snapshot: [T][N][A]; [T][N][A] (two heads) or [members][A]
    float *kl_pieces = nullptr;                 // [members][pg_slots][kPgKlPieces]
    // the shuffled sample-level minibatches / target-KL stop add-on of the live PPO / A2C trainer (adc_engine_pg_shuffle_init;
    // parts/kernel_pg_shuffle.inc, parts/pg_shuffle_api.inc; the law is adc_pg_shuffle.h).  Its device arrays are the trainer's too
    bool sh_live = false, sh_epoch_ready = false;
    int sh_mb = 0;                              // minibatch_samples
    uint32_t sh_ns = 0;                         // positions per member of the order last drawn
    std::vector<adc_pg_shuffle_config> sh_cfg;  // [members]
    std::vector<PgShuffleMember> sh_mem;        // [members] the host's copy of sh_dmem: the keys, the ticks of the order last drawn
    std::vector<adc_pg_shuffle_stats> sh_stats; // [members] of the update in progress / the last one
    std::vector<uint8_t> sh_evaluated;          // [members] the member was live when the last minibatch ran
    std::vector<int64_t> sh_last_count;         // [members] samples of the member's last evaluated minibatch
    PgShuffleMember *sh_dmem = nullptr;
    uint32_t *sh_order = nullptr, *sh_rows = nullptr;       // [members][T_max * envs of a member] each, packed [members][sh_ns]
    // the queued update of the live PPO / A2C trainer (adc_engine_pg_update_queued / _pg_pop_update_queued; parts/kernel_pg_queued.inc,
    // parts/pg_api.inc): one device block - the members' decision constants | step tables | the epochs' shuffle rows | control
    // blocks | the log - and its pinned twin on the host, allocated at the first queued update and grown on demand; the device
    // block is one of the trainer's allocations (pg_allocs), the host's goes in pg_drop
    uint8_t *pq_dev = nullptr, *pq_host = nullptr;
    size_t pq_bytes = 0;
    // off-policy training over a replay ring filled from the record (adc_engine_td3_init; parts/kernel_td3.inc, parts/td3_api.inc)
    bool have_td3 = false, td3_norm_set = false, td3_gap = false;
    bool td3_critic_set[2][4] = {{false, false, false, false}, {false, false, false, false}};
    adc_td3_config td3_cfg{};
    adc::Td3Shape td3_shape{};
    uint64_t td3_key = 0;
    int64_t td3_updates = 0, td3_actor_steps = 0, td3_written = 0;    // critic updates, actor steps, transitions stored so far
    int td3_stored_t = 0;               // the record's days [0, td3_stored_t) are in the ring
    int td3_Qc = 0, td3_P = 0;          // parameters of one critic, of the actor
    PgLayout td3_lay[4] = {};           // the flat orders against the stores: theta, psi, target theta, target psi
    MlpNet td3_q[2] = {}, td3_q_t[2] = {}, td3_pol_t{};
    float *td3_a_shift = nullptr, *td3_a_scale = nullptr;             // [A]
    Td3Ring td3_ring{};
    float *td3_flat[4] = {nullptr, nullptr, nullptr, nullptr};        // theta [P], psi [2 Qc], target theta, target psi
    float *td3_mom[4] = {nullptr, nullptr, nullptr, nullptr};         // Adam: m theta, v theta, m psi, v psi
    float *td3_grad = nullptr, *td3_ybuf = nullptr, *td3_xin = nullptr, *td3_acts = nullptr, *td3_deltas = nullptr, *td3_pieces = nullptr;
    int32_t *td3_idx = nullptr;         // [B] adc_engine_td3_batch_indices' device result
    double *td3_part = nullptr, *td3_sums = nullptr, *td3_gpart = nullptr;
    std::vector<void *> td3_allocs;
    // ... of a soft actor-critic learner (adc_engine_sac_init; parts/kernel_sac.inc, parts/sac_api.inc).  It shares the fields above -
    // the ring, the critics and their targets, the scratch, td3_flat / td3_mom (no target actor: [kTd3ThetaT] stays null), the
    // counters; td3_cfg holds the fields the shared helpers read (capacity, batch_size, the optimiser's, max_grad_norm)
    bool have_sac = false;
    adc_sac_config sac_cfg{};
    adc::SacLaw sac_law{};
    float *sac_cell = nullptr;          // {log_alpha, m, v, alpha} on the device (among td3_allocs)
    // ... and of a TD3 learner population (adc_engine_td3_pop_init; parts/kernel_td3_pop.inc, parts/td3_pop_api.inc).  It shares the
    // fields above, sized for all members at once: td3_flat / td3_mom are [M][P] or [M][2 Qc], the scratch [M][B][...], td3_sums
    // [M][16]; td3_cfg holds the fields all members share, td3_lay member 0's stores, the counters count for all (lock-step)
    bool have_td3_pop = false;
    std::vector<adc_td3_config> tp_cfg;         // [M]
    std::vector<Td3Member> tp_mem;              // [M] the host's copy of tp_dmem
    std::vector<Td3PopStep> tp_steps;           // [updates of a block][critic, actor][M] the host's copy of tp_dsteps
    std::vector<double> tp_host_sums;           // [M][16]
    std::vector<uint8_t> tp_critic_set;         // [M][2][4] uploaded since init
    Td3Member *tp_dmem = nullptr;
    Td3PopStep *tp_dsteps = nullptr;
    size_t tp_stride[4] = {0, 0, 0, 0};         // floats between two members' stores, per flat vector (theta's: lrn_stride)
    size_t tp_part_stride = 0;                  // doubles of chunk partials per member
    // ... and of a SAC learner population (adc_engine_sac_pop_init; parts/kernel_sac_pop.inc, parts/sac_pop_api.inc).  It lives in the
    // TD3 population's fields (no target actor: [kTd3ThetaT] stays null, Td3Member::pol_t empty; tp_cfg holds what the shared helpers
    // read of a member's configuration; tp_steps has three rows per update: critic, actor, temperature) under a flag of its own,
    // so that nothing that asks for a TD3 population (the TD3 normalisers, the PBT scheduler) takes it for one
    bool have_sac_pop = false;
    std::vector<adc_sac_config> sp_cfg;         // [M]
    std::vector<SacMember> sp_mem;              // [M] the host's copy of sp_dmem
    SacMember *sp_dmem = nullptr;
    float *sp_cells = nullptr;                  // [M][4] {log_alpha, m, v, alpha} on the device
    // the population-based training scheduler over the live pg_pop, td3_pop or sac_pop trainer (parts/pbt_api.inc; the law is adc_pbt.h).
    // Its device arrays are the trainer's allocations (pg_allocs / td3_allocs): they go with it
    bool have_pbt = false;
    int pbt_kind = 0;                           // adc_pbt_kind
    adc_pbt_config pbt_cfg{};
    uint64_t pbt_key = 0;
    int64_t pbt_round = 0;
    std::vector<double> pbt_s, pbt_host_fit;    // [M] the smoothed fitness; the fetched fitness
    std::vector<PbtPair> pbt_pairs;             // [M] the host's copy of pbt_dpairs
    double *pbt_ret = nullptr, *pbt_fit = nullptr;      // [N] the envs' returns, [M] the members' fitness
    PbtPair *pbt_dpairs = nullptr;
    // the running normalisers fed from the record (parts/kernel_norm.inc, parts/norm_api.inc).  on: the observation normaliser of
    // the PPO / A2C learners (adc_engine_obs_norm_init; the law is adc_norm.h).  rn: their reward normaliser (adc_engine_rew_norm_init;
    // adc_rew_norm.h), which lives with the trainer whose gamma it discounts by.  tn: the TD3 learners' normalisers
    // (adc_engine_td3_norm_init; adc_td3_norm.h), which live with the TD3 trainer; while tn.obs lives the record's obs rows (and so
    // the ring's) are raw observations.  sn: the SAC learners' normalisers (adc_engine_sac_norm_init; adc_sac_norm.h), which live with
    // the SAC trainer under the same rules; tn and sn never live together (one trainer owns the ring)
    NormSet on, rn, tn, sn;
    adc_obs_norm_config on_cfg{};
    adc_rew_norm_config rn_cfg{};
    adc_td3_norm_config tn_cfg{};
    adc_sac_norm_config sn_cfg{};
    // prioritised replay over the live TD3 / SAC trainer's ring(s), solo or population (adc_engine_replay_prio_init; parts/kernel_per.inc,
    // parts/per_api.inc; the law is adc_per.h).  Its device arrays are the trainer's allocations (td3_allocs): they go with it
    bool per_live = false;
    adc_replay_prio_config per_cfg{};
    PerView per{};                              // all members' trees, tops and batch buffers
    // n-step returns over the live TD3 / SAC trainer's ring(s) (adc_engine_replay_nstep_init; parts/nstep_api.inc; adc_td3.h "n-step").
    // nstep_n: the window, 0 while the add-on is off; nstep_gn: the members' gn arrays [M][C], among td3_allocs (the rings' gn point here)
    int nstep_n = 0;
    float *nstep_gn = nullptr;
    // how often the envs were stepped or reset, by anyone; ro_moves: that count when the record's last day was recorded
    uint64_t env_moves = 0, ro_moves = 0;
    bool ideal_full_scan = false;       // ADCRAFT_IDEAL_FULL_SCAN=1: evaluate the whole bid grid every step (the checker of the contender lists)
    // two consecutive days of the device-resident loop captured as one hipGraph (adc_engine_run_days)
    hipGraphExec_t day_graph = nullptr;
    bool day_graph_enabled = false;
    int day_graph_policy = -1, day_graph_parity = 0;
    float day_graph_budget = 0.0f;
    // everything the captured kernel nodes bake in by value: the graph is re-captured when any of it differs
    struct GraphKey { View v; PolicyView pol; InterpView ip; bool have_agent, have_curves, have_ideal, have_interp, lists, rest, direct; float mean_volume_hint; int fast_tiles_per_wg; } day_graph_key{};
    std::vector<void *> curve_allocs;   // ir / cpc / grid (re-allocated when the grid size changes)
    // the communicator of the episode-metric all-reduce (parts/comm_api.inc); null = this engine is alone
    void *comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    double *d_comm_vec = nullptr;
    size_t comm_vec_len = 0;
    hipEvent_t comm_ev[3] = {nullptr, nullptr, nullptr};      // adc_engine_metrics_allreduce: start | own reduction done | all-reduce done
    long long comm_calls = 0;
    double comm_ms_local = 0.0, comm_ms_collective = 0.0;
    hipEvent_t region_ev[2] = {nullptr, nullptr};             // adc_engine_region_begin / _end
};
int comm_release(adc_engine *e);       // parts/comm_api.inc

namespace {

constexpr int kMaxGroups = 4;
constexpr int kIdleRowsGrid = 32;       // workgroups of k_step_exact_rows while no budget has ever bound (launch_implicit)
// The streams of the env groups.  HIP multiplexes the streams of one priority onto FOUR hardware queues; a new stream is given the queue
// with the fewest streams on it (ties: the last one), for good - tools/microbench/stream_queues.hip prints the pairs that serialise.
// Two env groups on one queue run one after the other, which is slower than not grouping at all, and whether that happens depends on
// every stream the process has created before: group 0 on the engine's stream + three new streams was the fastest scheme measured
// until the null stream came into being (a hipMemcpyFromSymbol), after which every new engine had two groups on one queue (cfg2 at
// budget 1000: 0.45 -> 0.59 ms per step; one group: 0.54); four new streams back to back collide in the first engine of a process
// (the fourth lands on the third's queue); the highest-priority pool is a pool of its own and measured slower (profiles/
// r05_stream_groups.txt).  So the engine does not guess: the first time a step wants groups it creates candidate streams one at a
// time (up to a dozen), finds by a 150 us spin kernel on the candidate and on each stream kept so far whether they overlap, keeps
// four that mutually do (one per hardware queue) and destroys the rest - 15 to 50 ms, once per engine (stream creation is 3-4 ms).
// The engine's own stream carries no kernel of a grouped step, only the events that fork and join it.  Fewer than four queues
// (GPU_MAX_HW_QUEUES) -> as many groups as there are; one -> no groups.
constexpr int kGroupStreamCandidates = 12;
inline int pick_group_streams(adc_engine *e)
{
    const long long ticks = 150 * 100;              // 150 us of the 100 MHz wall clock
    auto spin_pair_us = [&](hipStream_t a, hipStream_t b) {
        (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b);
        const auto t0 = std::chrono::steady_clock::now();
        hipLaunchKernelGGL(k_spin_ticks, dim3(1), dim3(kWave), 0, a, ticks);
        if (b != a) hipLaunchKernelGGL(k_spin_ticks, dim3(1), dim3(kWave), 0, b, ticks);
        (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b);
        return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    };
    // candidates one at a time (creating a stream costs 3-4 ms, destroying one 2): usually the first four or five settle it
    hipStream_t rejected[kGroupStreamCandidates] = {};
    int kept = 0, n_rejected = 0;
    double alone = 0.0;
    for (int c = 0; c < kGroupStreamCandidates && kept < kMaxGroups; ++c) {
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); break; }
        if (c == 0) {
            (void)spin_pair_us(s, s);               // (the kernel's first launch: code object load)
            alone = std::min(spin_pair_us(s, s), spin_pair_us(s, s));
        }
        bool overlaps_all = true;
        for (int k = 0; k < kept && overlaps_all; ++k) {
            // (serialised: two spins; overlapped: one.  The smaller of two tries: a hiccup only ever makes a pair look serialised)
            const double us = std::min(spin_pair_us(e->gstream[k], s), spin_pair_us(e->gstream[k], s));
            overlaps_all = us < 1.5 * alone;       // (alone: one spin + the launch and synchronise overhead, ~170 us)
        }
        if (overlaps_all) e->gstream[kept++] = s;
        else rejected[n_rejected++] = s;
    }
    for (int c = 0; c < n_rejected; ++c) (void)hipStreamDestroy(rejected[c]);
    (void)hipGetLastError();
    return kept;
}

constexpr int kCounterInts = 16;        // flag_count, flag_next, xover_count, retry_count, rest_count, rest_next, direct_count, direct_next: [2] each

// one set of the lists' counters into a view (set 0: the engine's own view; 1 + g: group g's)
inline void point_counters(View &v, int *set)
{
    v.flag_count = set; v.flag_next = set + 2; v.xover_count = set + 4; v.retry_count = set + 6;
    v.rest_count = set + 8; v.rest_next = set + 10; v.direct_count = set + 12; v.direct_next = set + 14;
}

// how many env groups an IMPLICIT step runs as (1: the engine's own view on its own stream).  Measured (profiles/r05_stream_groups.txt,
// ms per device-resident step at 1 / 2 / 4 groups): cfg2 0.221 / 0.192 / 0.194 budget-free, 0.536 / 0.497 / 0.456 with every budget
// binding at 1000, 0.309 / 0.288 / 0.261 at 10; 4096 x 512 at 4000 1.54 / 1.28 / 1.25; 2048 x 1024 at 4000 1.06 / 0.96 / 0.90;
// 8192 x 1024 budget-free 1.472 / 1.460 / 1.455.  The sparse pass - long-lived workgroups that prefetch their next tile, the kernel
// nearest the HBM bound - has the least to gain: 16384 x 1024 sparse 0.457 / 0.447 / 0.454 at its four tiles per workgroup: two groups.
// ... and only for CHAINED steps - adc_engine_step_device following adc_engine_step_device with nothing in between: forking the groups
// off the engine's stream and joining them again costs 40-80 us of cross-queue signalling per step, more than the overlap inside one
// step returns (cfg2, ms per step at 1 / 2 / 4 groups when every step is joined: an agent kernel before each step 0.229 / 0.266 /
// 0.304, a synchronize after each 0.227 / 0.249 / 0.273, the same with every budget binding 0.549 / 0.577 / 0.604).  A chain of
// device-resident steps forks once and joins when the caller next asks for anything.
inline int stream_groups(adc_engine *e, const adc_engine::StepPlan &plan, bool chained)
{
    const int N = e->v.N, K = e->v.K;
    int G = 1;
    if (e->groups_override > 0) G = std::min(std::min(e->groups_override, kMaxGroups), N);
    else if (chained && N >= 2048 && K <= 1024) {
        const bool sparse = e->v.model == ADC_MODEL_IMPLICIT &&
                            (e->fast_variant == 2 || (e->fast_variant == 0 && e->mean_volume_hint >= 0.0f && e->mean_volume_hint < (float)kDenseVolumePerKeyword));
        // (the float-money models gain the same way - the default ImplicitKeyword 4096 x 256: 1.17 -> 1.02 ms budget-free, 1.75 -> 1.47
        //  binding; ExplicitKeyword 4096 x 512: 0.44 -> 0.39, 1.49 -> 1.31; 2048 x 1024: 0.46 -> 0.43, 2.27 -> 2.14 - except the default
        //  model beyond 512 keywords, whose 1024-lane workgroups already leave no tail: 1.34 -> 1.43)
        const bool wide_general = e->v.model == ADC_MODEL_IMPLICIT_GENERAL && K > 512;
        // (... and a budget-free IMPLICIT batch of many rounds of workgroups, whose tail is a few percent of the launch: 8192 x 1024 -
        //  25.6 rounds over the 1280 resident slots - 1.484 ms as one group, 1.501 as four in bench.py's runs; 2048 x 1024 - 6.4 rounds -
        //  0.378 -> 0.364.  Once a budget binds the small kernels are what the groups hide, whatever the batch)
        const long long rounds = (long long)N * ((K + kFastBlock - 1) / kFastBlock) / ((long long)e->num_cus * 5);
        const bool long_launch = e->v.model == ADC_MODEL_IMPLICIT && !sparse && rounds >= 16 && !plan.rest && !plan.lists;
        G = wide_general || long_launch ? 1 : sparse ? 2 : kMaxGroups;
    }
    if (G > 1 && e->group_streams == 0 && !e->no_group_streams) {
        // the groups' streams and events, the first time a step wants them (an engine of one env - a BiddingSimulation - never does)
        e->group_streams = pick_group_streams(e);
        bool ok = e->group_streams >= 2 && hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) == hipSuccess;
        for (int g = 0; g < e->group_streams && ok; ++g) ok = hipEventCreateWithFlags(&e->ev_join[g], hipEventDisableTiming) == hipSuccess;
        if (!ok) { (void)hipGetLastError(); e->no_group_streams = true; }      // (scheduling only: one group, for the life of the engine)
    }
    return G <= 1 || e->no_group_streams ? 1 : std::min(G, e->group_streams);
}

// the view of env group g of G: envs [e0, e0 + n) of the engine, every per-env pointer offset to e0 (null pointers stay null: the
// paths they stand for are off), the parameter planes still strided by the engine's N (View::NP), lists and counters of its own
inline View group_view(const adc_engine *e, int g, int G, int *e0_out)
{
    View v = e->v;
    const int N = e->v.N;
    const int e0 = (int)((long long)N * g / G), e1 = (int)((long long)N * (g + 1) / G);
    const size_t K = (size_t)v.K, o = (size_t)e0, ok = o * K;
    *e0_out = e0;
    v.N = e1 - e0;
    auto at = [](auto *&ptr, size_t off) { if (ptr) ptr += off; };
    at(v.params, ok);
    at(v.key, o); at(v.tick, o); at(v.day, o); at(v.cum_cents, o); at(v.cum, o); at(v.drift_pending, o); at(v.exact_hint, o);
    at(v.drift_bits, o * ((K + 31) / 32)); at(v.drift_rate, o * 3);
    at(v.flag_list, o); at(v.xover_list, o); at(v.retry_list, o);
    at(v.click_rec, o * kClickSegments * (size_t)v.click_cap); at(v.click_count, o * adc::kTimesteps); at(v.click_tick, o);
    at(v.click_row_hint, o); at(v.click_price_hint, o);
    at(v.rest_state, o); at(v.rest_counts, ok); at(v.rest_cost, ok); at(v.rest_rev, ok);
    at(v.rest_table, o * adc::kTimesteps * K); at(v.rest_marks, o * (size_t)v.rest_marks_stride); at(v.rest_nmarks, o);
    at(v.direct_budget, o); at(v.direct_list, o);
    at(v.gs_profit, ok); at(v.gs_spend, ok);
    at(v.env_cost, o); at(v.env_profit, o);
    at(v.imp, ok); at(v.clk, ok); at(v.conv, ok); at(v.cost, ok); at(v.rev, ok);
    at(v.reward, o); at(v.cum_profit, o); at(v.day_out, o); at(v.term, o); at(v.trunc, o);
    at(v.metric_env, o); at(v.metric_lo, ok); at(v.metric_hi, ok);
    at(v.flat_obs, o * (5 * K + 2));
    point_counters(v, e->d_counters + kCounterInts * (1 + g));
    return v;
}

// ... and of the policy state: the agent's caches and stream, the bid curves, the ideal sums, the contender lists of the same envs
inline PolicyView policy_group_view(const adc_engine *e, int g, int G)
{
    PolicyView p = e->pol;
    const int N = e->v.N;
    const int e0 = (int)((long long)N * g / G);
    const size_t K = (size_t)e->v.K, o = (size_t)e0, ok = o * K;
    auto at = [](auto *&ptr, size_t off) { if (ptr) ptr += off; };
    at(p.ave_rpc, ok); at(p.n_rpc, ok); at(p.ave_sctr, ok); at(p.n_sctr, ok); at(p.max_bid, ok);
    at(p.key, o); at(p.tick, o);
    at(p.curve, ok * (size_t)p.n_bids); at(p.xcurve, ok);
    at(p.ideal, ok); at(p.best, ok); at(p.sum_ideal, ok); at(p.sum_ideal_pos, ok);
    at(p.contender, ok * (size_t)p.cont_cap); at(p.n_contenders, ok); at(p.cont_pos, ok);
    return p;
}

// whatever rewrites the keyword parameters or the stream position ends the replayability of the steps before it
// (adc_engine_outcomes_replay recomputes the stream position and reads the parameters as they stand)
inline void forget_replayable_steps(adc_engine *e) { e->last_step = 0; e->stream_steps = 0; }

// the pending drift of every env into the parameter planes (what keyword_params shows after a step)
inline void materialize_drift(adc_engine *e)
{
    hipLaunchKernelGGL(k_materialize_drift, dim3(e->v.N), dim3(256), 0, e->stream, e->v);
    e->drift_applied = true;
}

constexpr size_t kSmallBlockBytes = 256 * 1024;      // engines whose outputs fit use single-copy host I/O

// (mlp_alloc of parts/mlp_core.inc is the learned agent's twin of this: owned by a list, and with a failure text of its own)
template <typename T>
int dev_alloc(adc_engine *e, T **p, size_t count)
{
    void *q = nullptr;
    hipError_t err = hipMalloc(&q, count * sizeof(T) > 0 ? count * sizeof(T) : sizeof(T));
    if (err != hipSuccess) return fail(ADC_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(err));
    e->allocs.push_back(q);
    err = hipMemsetAsync(q, 0, count * sizeof(T) > 0 ? count * sizeof(T) : sizeof(T), e->stream);
    if (err != hipSuccess) return fail(ADC_EHIP, std::string("hipMemsetAsync: ") + hipGetErrorString(err));
    *p = static_cast<T *>(q);
    return ADC_OK;
}

// The device temporaries of one call - host arrays staged for a kernel, scratch a result is copied out of - on the stream the call
// works on.  get allocates, up allocates and enqueues the upload; neither words an error: the call site has its own sentence.
// release() frees them, and stands where the call has just waited for that stream itself.  A call that returns before it leaves
// them to the destructor, which waits for the stream first: nothing is freed under a copy or a kernel in flight, and nothing
// relies on hipFree's own wait.
struct DevTemps {
    hipStream_t stream;
    std::vector<void *> held;
    explicit DevTemps(hipStream_t s) : stream(s) {}
    DevTemps(const DevTemps &) = delete;
    DevTemps &operator=(const DevTemps &) = delete;
    ~DevTemps()
    {
        if (held.empty()) return;
        (void)hipStreamSynchronize(stream);
        release();
    }
    template <typename T>
    hipError_t get(T **p, size_t bytes)
    {
        const hipError_t err = hipMalloc((void **)p, bytes);
        if (err == hipSuccess) held.push_back(*p);
        return err;
    }
    template <typename T>
    hipError_t up(T **p, const void *host, size_t bytes)
    {
        const hipError_t err = get(p, bytes);
        return err != hipSuccess ? err : hipMemcpyAsync(*p, host, bytes, hipMemcpyHostToDevice, stream);
    }
    void release()
    {
        for (void *q : held) (void)hipFree(q);
        held.clear();
    }
};

int flush_profile(adc_engine *e)
{
    for (int i = 0; i < e->ev_used; ++i) {
        hipEvent_t *m = &e->ev[(size_t)i * kProfileMarks];
        HIP_TRY(hipEventSynchronize(m[kProfileMarks - 1]));
        for (int j = 0; j < 3; ++j) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, m[j], m[j + 1]));
            e->prof_ms[j] += ms;
        }
        e->prof_launches += 1;
    }
    e->ev_used = 0;
    return ADC_OK;
}

// mean of the vol_mean plane, taken on the device once after the keyword parameters changed (one small reduction and a
// synchronisation at the first step after a reset / upload; drift moves it by a few percent per episode and is ignored)
int refresh_volume_hint(adc_engine *e)
{
    e->volume_hint_dirty = false;
    if (!e->d_hint_sum) {
        if (hipMalloc((void **)&e->d_hint_sum, sizeof(double)) != hipSuccess) { e->mean_volume_hint = -1.0f; return ADC_OK; }
        e->allocs.push_back(e->d_hint_sum);
    }
    const size_t nk = (size_t)e->v.N * e->v.K;
    HIP_TRY(hipMemsetAsync(e->d_hint_sum, 0, sizeof(double), e->stream));
    hipLaunchKernelGGL(k_sum_plane, dim3((unsigned)std::min<size_t>((nk + 1023) / 1024, 1024)), dim3(256), 0, e->stream, e->v.params + (size_t)ADC_P_VOL_MEAN * nk, nk,
                       e->d_hint_sum);
    HIP_TRY(hipGetLastError());
    double sum = 0.0;
    HIP_TRY(hipMemcpyAsync(&sum, e->d_hint_sum, sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->mean_volume_hint = (float)(sum / (double)nk);
    return ADC_OK;
}

// Which optional kernels the next IMPLICIT step launches - the listing variant of the fast pass, the rest-of-day kernels behind the row
// kernel, their at-once variant - decided ONCE per step from the three page-locked words the device sets, before anything of the step is
// enqueued or counted; the two big buffers those paths need (the click lists' records: 840 MB at 4096 x 256; the table
// k_step_rest_of_day<true> hands to k_rest_walk: 100 MB) are allocated here, the first time the device asks for them.  Both paths
// are scheduling choices (the row kernel alone gives the same results), so an allocation that fails turns its path off for the
// life of the engine instead of failing the step: nothing of the step has happened yet, and nothing of it depends on the buffer.
// Not inside a stream capture: adc_engine_run_days plans before it captures and hands the plan in (capture_plan).  A stale read of a
// flag word only delays a path by a step.
adc_engine::StepPlan plan_step(adc_engine *e)
{
    if (e->in_capture) return e->capture_plan;
    adc_engine::StepPlan p{false, false, false};
    auto flagged = [](const int *word) { return word && *reinterpret_cast<const volatile int *>(word) != 0; };
    auto lazy_alloc = [&](void **q, size_t bytes, int fill) {
        *q = nullptr;
        hipError_t err = e->fail_lazy_alloc ? hipErrorOutOfMemory : hipMalloc(q, bytes);
        if (err == hipSuccess) {
            err = hipMemsetAsync(*q, fill, bytes, e->stream);
            if (err == hipSuccess) { e->allocs.push_back(*q); e->needs_fork = true; return true; }      // (cleared on the engine's stream: the env groups wait for it)
            (void)hipFree(*q);
            *q = nullptr;
        }
        (void)hipGetLastError();            // (not an error of the step: do not leave it for the next check)
        return false;
    };
    if (e->click_rec_count && !e->v.click_rec && flagged(e->h_listing)) {
        void *q = nullptr;
        if (lazy_alloc(&q, e->click_rec_count * sizeof(uint2), 0)) e->v.click_rec = static_cast<uint2 *>(q);
        else { e->click_rec_count = 0; e->v.click_count = nullptr; }     // the path is off from this step on (View::click_count == null: as for K > 256):
                                                                           // envs that were listing go through the row kernel and get hint 2 / 6 there
    }
    p.lists = e->v.click_rec != nullptr;
    p.rest = flagged(e->h_binding);
    if (p.rest && e->rest_table_count && !e->v.rest_table) {
        void *q = nullptr;
        if (lazy_alloc(&q, e->rest_table_count * sizeof(unsigned short), 0xFF)) e->v.rest_table = static_cast<unsigned short *>(q);
        else { e->rest_table_count = 0; e->h_binding_off = true; }
    }
    if (e->h_binding_off) p.rest = false;   // the pair of kernels cannot run without its table: the row kernel finishes its days itself
    p.direct = p.rest && flagged(e->h_direct);
    return p;
}

// the engine's stream waits for everything its env groups have in flight (one event per group); a no-op when nothing is
inline int join_groups(adc_engine *e)
{
    if (!e->groups_pending) return ADC_OK;
    for (int g = 0; g < e->last_groups; ++g) {
        HIP_TRY(hipEventRecord(e->ev_join[g], e->gstream[g]));
        HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_join[g], 0));
    }
    e->groups_pending = false;
    return ADC_OK;
}

// The IMPLICIT step of the envs of one View on one stream: the keyword-parallel pass, k_tail_or_flag, and whatever the plan says the
// budget-exact paths need.  `v` is the engine's own view (all envs, the engine's stream) or the view of an env GROUP (group_view)
// on the group's stream; d_bids / d_budget are that view's first env's.  mark (nullable): profiling events of the engine's stream.
int launch_implicit(adc_engine *e, const View &v, hipStream_t st, const float *d_bids, const float *d_budget, const adc_engine::StepPlan &plan,
                    int parity, bool prof, hipEvent_t *mark)
{
    const int N = v.N, K = v.K;
    const size_t lds = (size_t)K * (4 * 4 + 3 * 8);
    TapeView none{};
    {
        // keywords per workgroup: one per lane, or fewer while that leaves most of the chip without a workgroup
        int tile_kw = kFastBlock;
        while (tile_kw > 16 && (long long)N * ((K + tile_kw - 1) / tile_kw) < e->num_cus) tile_kw >>= 1;
        if (e->fast_tile_kw > 0) tile_kw = e->fast_tile_kw;             // ADCRAFT_FAST_TILE_KW (measurements)
        const int tiles = (K + tile_kw - 1) / tile_kw;
        // tiles per workgroup: 1 while the grid is a few workgroups per resident slot (big tiles: let the dispatcher balance);
        // small tiles (sparse keyword sets) are taken several at a time - parameters prefetched, tables copied once
        // (chosen from the ENGINE's tile count: an env group takes the tiles per workgroup the whole batch would - halving them with the
        //  group's size is what made the sparse pass slower in groups: cfg3 at 2 groups 0.470 ms with 2 tiles, 0.447 with 4)
        const long long n_tiles = (long long)N * tiles;
        int per_wg = e->fast_tiles_per_wg;
        if (per_wg <= 0) {
            per_wg = 1;
            const long long slots = (long long)e->num_cus * 5, engine_tiles = (long long)v.NP * tiles;
            if (e->mean_volume_hint >= 0.0f && e->mean_volume_hint < 32.0f)
                while (per_wg < 8 && engine_tiles / (per_wg * 2) >= 8 * slots) per_wg *= 2;
        }
        const unsigned grid = (unsigned)((n_tiles + per_wg - 1) / per_wg);
        // few auctions per keyword (sparse keyword sets): the variant without interval records (a hint: both are exact)
        const bool sparse = e->fast_variant == 2 || (e->fast_variant == 0 && e->mean_volume_hint >= 0.0f && e->mean_volume_hint < (float)kDenseVolumePerKeyword);
        // (the variant that lists clicked wins, once the device has said that some env wants them: a stale read only delays it)
        const bool lists = plan.lists;
        e->step_kernel = tile_kw != kFastBlock ? (lists ? "k_step_implicit_fast<true, lists>" : "k_step_implicit_fast<true>")
                         : sparse              ? "k_step_implicit_sparse"
                         : lists               ? "k_step_implicit_fast<false, lists>"
                                               : "k_step_implicit_fast<false>";
        if (tile_kw == kFastBlock) {
            if (sparse) hipLaunchKernelGGL(k_step_implicit_sparse, dim3(grid), dim3(kFastBlock), 0, st, v, d_bids, per_wg);
            else if (lists) hipLaunchKernelGGL((k_step_implicit_fast<false, true>), dim3(grid), dim3(kFastBlock), 0, st, v, d_bids, tile_kw, per_wg);
            else hipLaunchKernelGGL((k_step_implicit_fast<false, false>), dim3(grid), dim3(kFastBlock), 0, st, v, d_bids, tile_kw, per_wg);
        } else if (lists) {   // a handful of envs: narrow tiles (the interval variant decides per tile how to resolve it)
            hipLaunchKernelGGL((k_step_implicit_fast<true, true>), dim3(grid), dim3(kFastBlock), 0, st, v, d_bids, tile_kw, per_wg);
        } else {
            hipLaunchKernelGGL((k_step_implicit_fast<true, false>), dim3(grid), dim3(kFastBlock), 0, st, v, d_bids, tile_kw, per_wg);
        }
        HIP_TRY(hipGetLastError());
        if (prof) HIP_TRY(hipEventRecord(mark[1], st));
        if (K <= kRowsMaxK) {
            // lanes per workgroup of the row kernel: 256 up to 512 keywords, 512 beyond (two workgroups of 512 lanes per CU hold the tables of
            // 1024 keywords: 128 registers, no spill).  A lane per keyword beyond 256 keywords (512 / 1024 lanes) was measured slower at
            // 2048 x 1024 and a wash at 4096 x 512 (one workgroup per CU idles while wave 0 resolves a row) and was removed in round 5:
            // profiles/HISTORY.md
            const int rows_block = K <= 512 ? kRowsBlock : 512;
            const bool rows_one = K <= kRowsBlock;
            const size_t lds_rows = (size_t)K * (5 * 8 + 8 * 4 + 1) + (rows_block / kWave) * kRowsRing * 4 + 16;
            // (k_step_rest_of_day behind the row kernel once that has reported a budget that binds: a stale read only delays it)
            bool rest = plan.rest;
            // (a handful of envs that list their clicked wins: the walk over the lists does their binding days, and a launch that finds
            //  nothing parked is 4 us of a 50-us step - what the lists cannot take, the row kernel finishes itself)
            if (lists && N <= 64) rest = false;
            // (... and k_step_rest_of_day<true, true> once k_rest_walk has reported an env for it)
            const bool direct = rest && plan.direct;
            hipLaunchKernelGGL(k_tail_or_flag, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, v, d_budget, parity, (!(sparse && tile_kw == kFastBlock) && !lists) ? 1 : 0,
                               direct ? 1 : 0);
            HIP_TRY(hipGetLastError());
            if (lists) {            // envs whose clicked wins the fast pass listed: the budget walk over the lists (persistent grid)
                hipLaunchKernelGGL(k_step_click_walk, dim3((unsigned)std::min(N, e->num_cus * 3)), dim3(kWalkBlock), 0, st, v, d_bids, d_budget, parity);
                HIP_TRY(hipGetLastError());
            }
            // persistent grid: as many workgroups as can be resident (registers / LDS), never more than envs
            if (e->rows_per_cu == 0) {
                int nb = 0;
                const hipError_t oe = rows_one          ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_step_exact_rows<true>, kRowsBlock, lds_rows)
                                      : rows_block == 512 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_step_exact_rows<false, 512>, 512, lds_rows)
                                                          : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_step_exact_rows<false>, kRowsBlock, lds_rows);
                if (oe != hipSuccess) (void)hipGetLastError();      // not an error of ours: do not leave it for the next check
                if (oe != hipSuccess || nb < 1) nb = 1;
                e->rows_per_cu = nb;
            }
            // (a few workgroups per resident slot: the hardware dispatcher balances better than the ticket loop alone; while the
            //  device has never reported a budget that binds - the bench - 32 workgroups: thousands of workgroups that find an empty
            //  list cost microseconds of every step - 256 of them still 7 us of cfg2's 215, more inside a chain of env groups, where
            //  they queue for slots behind another group's auctions - and the ticket loop takes whatever the first binding step
            //  brings: that one step is slow, the word it sets brings the full grid from the next step on)
            const bool binds = rest || !e->h_binding || lists;
                        const int grid = std::min(N, binds ? 4 * e->num_cus * e->rows_per_cu : kIdleRowsGrid);
            if (rows_one) hipLaunchKernelGGL(k_step_exact_rows<true>, dim3((unsigned)grid), dim3(kRowsBlock), lds_rows, st, v, d_bids, d_budget, parity, rest ? 1 : 0);
            else if (rows_block == 512) hipLaunchKernelGGL((k_step_exact_rows<false, 512>), dim3((unsigned)grid), dim3(512), lds_rows, st, v, d_bids, d_budget, parity, rest ? 1 : 0);
            else hipLaunchKernelGGL(k_step_exact_rows<false>, dim3((unsigned)grid), dim3(kRowsBlock), lds_rows, st, v, d_bids, d_budget, parity, rest ? 1 : 0);
            if (rest) {             // the rest of the days it parked (persistent grid)
                HIP_TRY(hipGetLastError());
                // (as many workgroups as can be resident, no more: with nothing parked every one of them still has to be given its LDS)
                const int rest_per_cu = std::max(1, std::min(6, (int)(160 * 1024 / (rest_lds_bytes(K) + 1024))));
                if (v.rest_marks) {
                    if (K > 512)      // (512 lanes: three workgroups of them per CU hold the tables of 1024 keywords)
                        hipLaunchKernelGGL((k_step_rest_of_day<true, false, 512>), dim3((unsigned)std::min(N, e->num_cus * 3)), dim3(512), (size_t)adc::kTimesteps * K * 2, st, v, d_bids, parity);
                    else
                        hipLaunchKernelGGL(k_step_rest_of_day<true>, dim3((unsigned)std::min(N, e->num_cus * kRestPassBlocks)), dim3(kRowsBlock), (size_t)adc::kTimesteps * K * 2, st, v, d_bids, parity);
                    HIP_TRY(hipGetLastError());
                    if (direct) {
                        hipLaunchKernelGGL((k_step_rest_of_day<true, true>), dim3((unsigned)std::min(N, e->num_cus * kRestFreshBlocks)), dim3(kRowsBlock), (size_t)adc::kTimesteps * K * 2, st, v, d_bids, parity);
                        HIP_TRY(hipGetLastError());
                    }
                    hipLaunchKernelGGL(k_rest_walk, dim3((unsigned)std::min(N, e->num_cus * 16)), dim3(kWave), 0, st, v, d_bids, d_budget, parity, direct ? 1 : 0);
                } else
                    hipLaunchKernelGGL(k_step_rest_of_day<false>, dim3((unsigned)std::min(N, e->num_cus * rest_per_cu)), dim3(kRowsBlock), rest_lds_bytes(K), st, v, d_bids, parity);
            }
        } else {
            hipLaunchKernelGGL((k_step_exact<ADC_MODEL_IMPLICIT, false>), dim3(N), dim3(kWave), lds, st, v, d_bids, d_budget, none, 1, ReplayOut{});
        }
    }
    return ADC_OK;
}

// The step of the two float-money models (the default ImplicitKeyword with its bidder pools, ExplicitKeyword) for the envs of one View
// on one stream - the engine's own view, or an env group's (group_view): keyword-parallel pass, then the budget-exact kernels over
// the envs it flagged.  mark (nullable): profiling events of the engine's stream.
int launch_float_models(adc_engine *e, const View &v, hipStream_t st, const float *d_bids, const float *d_budget, int parity, bool prof, hipEvent_t *mark)
{
    const int N = v.N, K = v.K;
    const size_t lds = (size_t)K * (4 * 4 + 3 * 8);
    TapeView none{};
    if (v.model == ADC_MODEL_IMPLICIT_GENERAL) {
        // the default ImplicitKeyword: keyword-parallel pass (exact unless the budget may bind), then the reference-order walker
        // (one wavefront per env; tens of bidders per auction) for the envs it flagged
        if (v.gs_profit) {
            // a handful of envs: a wavefront per keyword (one workgroup walking an env's keywords, a lane each, is latency-bound: 218 us
            // per step for one env x 100 keywords), then the env's tail in a second, tiny launch
            e->step_kernel = "k_step_general_small";
            hipLaunchKernelGGL(k_step_general_small, dim3((unsigned)(((size_t)N * K + 3) / 4)), dim3(256), 0, st, v, d_bids);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_general_small_tail, dim3((unsigned)N), dim3(kWave), (size_t)K * 8, st, v, d_budget, parity);
        } else {
            e->step_kernel = "k_step_general_fast";
            hipLaunchKernelGGL(k_step_general_fast, dim3((unsigned)N), dim3(256), (size_t)K * 8, st, v, d_bids, d_budget, parity);
        }
        HIP_TRY(hipGetLastError());
        if (prof) HIP_TRY(hipEventRecord(mark[1], st));
        if (K <= kXDayKMax) {
            // flagged days by keyword-parallel click lists + one float64 walk per row (lane = keyword: 256, 512 or 1024 lanes);
            // what that cannot hold goes on to the walker
            if (K <= kXDayK) hipLaunchKernelGGL((k_step_float_day<ADC_MODEL_IMPLICIT_GENERAL, kXDayK>), dim3(N), dim3(kXDayK), 0, st, v, d_bids, d_budget, parity);
            else if (K <= 512) hipLaunchKernelGGL((k_step_float_day<ADC_MODEL_IMPLICIT_GENERAL, 512>), dim3(N), dim3(512), 0, st, v, d_bids, d_budget, parity);
            else hipLaunchKernelGGL((k_step_float_day<ADC_MODEL_IMPLICIT_GENERAL, 1024>), dim3(N), dim3(1024), 0, st, v, d_bids, d_budget, parity);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL((k_step_exact<ADC_MODEL_IMPLICIT_GENERAL, false>), dim3(N), dim3(kWave), lds, st, v, d_bids, d_budget, none, 5 + parity, ReplayOut{});
        } else {
            hipLaunchKernelGGL((k_step_exact<ADC_MODEL_IMPLICIT_GENERAL, false>), dim3(N), dim3(kWave), lds, st, v, d_bids, d_budget, none, 3 + parity, ReplayOut{});
        }
    } else {
        // keyword-parallel pass (exact unless the budget may bind), then the serial walker for the envs it flagged
        e->step_kernel = "k_step_explicit_fast";
        hipLaunchKernelGGL(k_step_explicit_fast, dim3((unsigned)N), dim3(256), (size_t)K * 8, st, v, d_bids, d_budget, parity);
        HIP_TRY(hipGetLastError());
        if (prof) HIP_TRY(hipEventRecord(mark[1], st));
        const size_t lds_xrows = (size_t)K * 48 + (size_t)kWave * kXMaxClicks * 9;
        if (lds_xrows <= 150 * 1024) {
            if (K <= kXDayKMax) {
                // whole flagged days by keyword-parallel click lists + one float64 walk (lane = keyword: 256, 512 or 1024 lanes);
                // what that cannot hold goes on to the row walker
                if (K <= kXDayK) hipLaunchKernelGGL((k_step_float_day<ADC_MODEL_EXPLICIT, kXDayK>), dim3(N), dim3(kXDayK), 0, st, v, d_bids, d_budget, parity);
                else if (K <= 512) hipLaunchKernelGGL((k_step_float_day<ADC_MODEL_EXPLICIT, 512>), dim3(N), dim3(512), 0, st, v, d_bids, d_budget, parity);
                else hipLaunchKernelGGL((k_step_float_day<ADC_MODEL_EXPLICIT, 1024>), dim3(N), dim3(1024), 0, st, v, d_bids, d_budget, parity);
                HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(k_step_explicit_rows, dim3(N), dim3(kWave), lds_xrows, st, v, d_bids, d_budget, parity, v.retry_list, v.retry_count);
            } else {
                hipLaunchKernelGGL(k_step_explicit_rows, dim3(N), dim3(kWave), lds_xrows, st, v, d_bids, d_budget, parity, v.flag_list, v.flag_count);
            }
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL((k_step_exact<ADC_MODEL_EXPLICIT, false>), dim3(N), dim3(kWave), lds, st, v, d_bids, d_budget, none, 1 + parity, ReplayOut{});
        } else {        // K > ~3000: the row walker's LDS does not fit; flagged envs go straight to the serial walker
            hipLaunchKernelGGL((k_step_exact<ADC_MODEL_EXPLICIT, false>), dim3(N), dim3(kWave), lds, st, v, d_bids, d_budget, none, 3 + parity, ReplayOut{});
        }
    }
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}

int launch_step(adc_engine *e, const float *d_bids, const float *d_budget, const TapeView *tape, bool lazy_join = false)
{
    View &v = e->v;
    const int N = v.N, K = v.K;
    const bool implicit = v.model == ADC_MODEL_IMPLICIT;
    const size_t lds = (size_t)K * (4 * 4 + 3 * 8);
    if (lds > 160 * 1024) return fail(ADC_EINVAL, "num_keywords too large for the exact pass (LDS)");
    // (before any launch and any bookkeeping: what this step will launch, and the lazy allocations behind it - plan_step)
    const adc_engine::StepPlan plan = (implicit && !tape) ? plan_step(e) : adc_engine::StepPlan{false, false, false};
    // (only adc_engine_step_device's steps may follow each other without the groups waiting for the engine's stream again: every other
    //  caller - the host step's uploads, adc_engine_run_days' policy kernels between two days - has just enqueued the step's inputs there)
    if (!lazy_join) e->needs_fork = true;
    const bool chained = lazy_join && !e->api_since_step && !e->stream_exposed;
    e->api_since_step = !lazy_join;
    e->last_step = tape ? 2 : 1;
    e->stream_steps = tape ? 0 : e->stream_steps + 1;
    e->env_moves += 1;
    e->drift_applied = false;
    if (tape) {
        e->step_kernel = "k_step_exact";
        if (implicit) hipLaunchKernelGGL((k_step_exact<ADC_MODEL_IMPLICIT, true>), dim3(N), dim3(kWave), lds, e->stream, v, d_bids, d_budget, *tape, 0, ReplayOut{});
        else if (v.model == ADC_MODEL_IMPLICIT_GENERAL) hipLaunchKernelGGL((k_step_exact<ADC_MODEL_IMPLICIT_GENERAL, true>), dim3(N), dim3(kWave), lds, e->stream, v, d_bids, d_budget, *tape, 0, ReplayOut{});
        else hipLaunchKernelGGL((k_step_exact<ADC_MODEL_EXPLICIT, true>), dim3(N), dim3(kWave), lds, e->stream, v, d_bids, d_budget, *tape, 0, ReplayOut{});
        HIP_TRY(hipGetLastError());
        if (v.flat_obs) {
            hipLaunchKernelGGL(k_flatten_obs, dim3((unsigned)((K + 255) / 256), (unsigned)N), dim3(256), 0, e->stream, v);
            HIP_TRY(hipGetLastError());
        }
        return ADC_OK;
    }
    const bool prof = e->profiling && (e->profile_tick++ % (unsigned)e->profile_every) == 0u;
    if (prof && e->ev_used == kProfileRing) { int rc = flush_profile(e); if (rc) return rc; }
    hipEvent_t *mark = prof ? &e->ev[(size_t)e->ev_used * kProfileMarks] : nullptr;
    if (prof) HIP_TRY(hipEventRecord(mark[0], e->stream));
    if (implicit && e->volume_hint_dirty && !(e->fast_tiles_per_wg && e->fast_variant)) { int rc = refresh_volume_hint(e); if (rc) return rc; }
    // One launch sequence for the envs of one view on one stream (the keyword-parallel pass, then the budget-exact kernels of its model)
    const int parity = (int)(e->step_serial++ & 1u);
    auto launch_model = [&](const View &view, hipStream_t st, const float *bids, const float *budget, bool with_marks) {
        return implicit ? launch_implicit(e, view, st, bids, budget, plan, parity, with_marks, with_marks ? mark : nullptr)
                        : launch_float_models(e, view, st, bids, budget, parity, with_marks, with_marks ? mark : nullptr);
    };
    const int G = prof || e->in_capture ? 1 : stream_groups(e, plan, chained);
    if (G != e->last_groups) {
        // (the lists' counters are double-buffered by step parity and cleared by the step before: a change of grouping starts from clean ones)
        { int rc = join_groups(e); if (rc) return rc; }
        HIP_TRY(hipMemsetAsync(e->d_counters, 0, sizeof(int) * kCounterInts * (1 + kMaxGroups), e->stream));
        e->last_groups = G;
        e->needs_fork = true;
    }
    if (G > 1) {
        // ENV GROUPS: the envs in G contiguous groups, each with its own view, lists and stream.  Their kernels run side by side - one
        // group's small, latency-bound kernels (the step tail, the budget-exact kernels at 56 % VALU occupancy) under another group's
        // keyword-parallel pass - and, device-resident steps following each other, a group starts its next step while another finishes
        // this one: the group streams wait for the engine's stream only when something was enqueued there since (needs_fork), and the
        // engine's stream waits for the groups when the next thing is enqueued on it (join_groups: every entry point that is not part
        // of a chain does it first).  Results do not depend on G.
        if (e->needs_fork || e->stream_exposed) {
            HIP_TRY(hipEventRecord(e->ev_fork, e->stream));
            for (int g = 0; g < G; ++g) HIP_TRY(hipStreamWaitEvent(e->gstream[g], e->ev_fork, 0));
            e->needs_fork = false;
        }
        for (int g = 0; g < G; ++g) {
            int e0 = 0;
            const View vg = group_view(e, g, G, &e0);
            int rc = launch_model(vg, e->gstream[g], d_bids + (size_t)e0 * K, d_budget + e0, false);
            if (rc) return rc;
            if (v.metrics_on && !implicit) {      // (see below: the float-money models' cent sums are a pass of their own)
                hipLaunchKernelGGL(k_metric_accumulate, dim3((unsigned)(((size_t)vg.N * K + 255) / 256)), dim3(256), 0, e->gstream[g], vg);
                HIP_TRY(hipGetLastError());
            }
        }
        e->groups_pending = true;
        if (!lazy_join || e->stream_exposed || v.flat_obs) { int rc = join_groups(e); if (rc) return rc; }      // (k_flatten_obs reads every group's outputs)
        if (v.flat_obs) {
            hipLaunchKernelGGL(k_flatten_obs, dim3((unsigned)((K + 255) / 256), (unsigned)N), dim3(256), 0, e->stream, v);
            HIP_TRY(hipGetLastError());
        }
        return ADC_OK;
    }
    { int rc = join_groups(e); if (rc) return rc; }
    { int rc = launch_model(v, e->stream, d_bids, d_budget, prof); if (rc) return rc; }
    e->needs_fork = true;                   // (a later grouped step is ordered behind this one)
    HIP_TRY(hipGetLastError());
    if (prof) HIP_TRY(hipEventRecord(mark[2], e->stream));
    if (v.metrics_on && !implicit) {      // the IMPLICIT kernels accumulate exact cents in their output phase; EXPLICIT money is float dollars
        const size_t nk = (size_t)N * K;
        hipLaunchKernelGGL(k_metric_accumulate, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, e->stream, v);
        HIP_TRY(hipGetLastError());
    }
    if (v.flat_obs) {
        hipLaunchKernelGGL(k_flatten_obs, dim3((unsigned)((K + 255) / 256), (unsigned)N), dim3(256), 0, e->stream, v);
        HIP_TRY(hipGetLastError());
    }
    if (prof) { HIP_TRY(hipEventRecord(mark[3], e->stream)); e->ev_used++; e->event_records += kProfileMarks; }
    return ADC_OK;
}

// every buffer of *out is page-locked host memory the device can address (hipHostMalloc / adc_host_alloc) and aligned for
// k_outputs_to_host; the answer is remembered per distinct set of pointers
bool outputs_device_addressable(adc_engine *e, const adc_step_out *out)
{
    if (std::memcmp(&e->checked_out, out, sizeof(*out)) == 0) return e->checked_out_ok;
    e->checked_out = *out;
    e->checked_out_ok = false;
    if (out->counts_u16 && (out->impressions || out->buyside_clicks || out->sellside_conversions)) return false;
    const void *const wide[5] = {out->impressions, out->buyside_clicks, out->sellside_conversions, out->cost, out->revenue};
    for (const void *p : wide)
        if ((uintptr_t)p & 15) return false;
    if ((uintptr_t)out->counts_u16 & 7) return false;
    const void *const all[12] = {out->impressions, out->buyside_clicks, out->sellside_conversions, out->cost, out->revenue, out->reward,
                                 out->cumulative_profit, out->days_passed, out->terminated, out->truncated, out->counts_u16, out->counts_overflow};
    for (const void *p : all) {
        if (!p) continue;
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }      // pageable memory
        if (attr.type != hipMemoryTypeHost || !attr.devicePointer || attr.devicePointer != p) return false;
    }
    return e->checked_out_ok = true;
}

constexpr int kDirectOutBlocks = 256;       // grid of k_outputs_to_host (page-locked, 16-byte aligned output buffers: the device writes them itself)

int fetch(adc_engine *e, adc_step_out *out, bool sync = true)
{
    const View &v = e->v;
    const size_t nk = (size_t)v.N * v.K, n = (size_t)v.N;
    if (out && (v.K & 3) == 0 && outputs_device_addressable(e, out)) {
        const HostOut h = {out->impressions, out->buyside_clicks, out->sellside_conversions, out->counts_u16, out->cost, out->revenue,
                           out->reward, out->cumulative_profit, out->days_passed, out->terminated, out->truncated, out->counts_overflow};
        if (out->counts_overflow) *out->counts_overflow = 0;        // (host write, ordered before the launch)
        const unsigned blocks = (unsigned)std::min<size_t>((nk / 4 + 255) / 256, (size_t)kDirectOutBlocks);
        hipLaunchKernelGGL(k_outputs_to_host, dim3(std::max(1u, blocks)), dim3(256), 0, e->stream, v, h);
        HIP_TRY(hipGetLastError());
        if (sync) HIP_TRY(hipStreamSynchronize(e->stream));
        return ADC_OK;
    }
    if (out && e->h_out_block && sync && !out->counts_u16) {
        HIP_TRY(hipMemcpyAsync(e->h_out_block, e->d_out_block, e->out_block_bytes, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        void *const dst[10] = {out->impressions, out->buyside_clicks, out->sellside_conversions, out->cost, out->revenue,
                               out->reward, out->cumulative_profit, out->days_passed, out->terminated, out->truncated};
        const size_t sizes[10] = {nk * 4, nk * 4, nk * 4, nk * 4, nk * 4, n * 8, n * 8, n * 4, n, n};
        for (int i = 0; i < 10; ++i)
            if (dst[i]) std::memcpy(dst[i], e->h_out_block + e->out_off[i], sizes[i]);
        return ADC_OK;
    }
    if (out && out->counts_u16) {
        if (v.K & 1) return fail(ADC_EINVAL, "counts_u16 needs an even num_keywords");
        if (!e->d_counts_u16) {
            int rc = dev_alloc(e, &e->d_counts_u16, 3 * nk);
            if (!rc) rc = dev_alloc(e, &e->d_counts_overflow, 1);
            if (rc) return rc;
        }
        HIP_TRY(hipMemsetAsync(e->d_counts_overflow, 0, sizeof(int), e->stream));
        hipLaunchKernelGGL(k_pack_counts, dim3((unsigned)((nk / 2 + 255) / 256)), dim3(256), 0, e->stream, v, e->d_counts_u16, e->d_counts_overflow);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out->counts_u16, e->d_counts_u16, 3 * nk * 2, hipMemcpyDeviceToHost, e->stream));
        if (out->counts_overflow) HIP_TRY(hipMemcpyAsync(out->counts_overflow, e->d_counts_overflow, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    }
    if (out) {
        // ten outputs = ten slices of one device block: host buffers laid out like the block (adc_engine_out_offsets) come back
        // in one transfer (21 MB: 0.38 ms as one, 0.46 ms as ten).  [a 2-D transfer for equally strided planes was tried and
        // is slower than one transfer per plane on this stack]
        struct Piece { char *dst; const char *src; size_t bytes; };
        void *const dst[10] = {out->impressions, out->buyside_clicks, out->sellside_conversions, out->cost, out->revenue,
                               out->reward, out->cumulative_profit, out->days_passed, out->terminated, out->truncated};
        const size_t sizes[10] = {nk * 4, nk * 4, nk * 4, nk * 4, nk * 4, n * 8, n * 8, n * 4, n, n};
        Piece p[10];
        int np = 0;
        for (int i = 0; i < 10; ++i) {
            if (!dst[i]) continue;
            const Piece q = {(char *)dst[i], (const char *)e->d_out_block + e->out_off[i], sizes[i]};
            if (np && q.dst - p[np - 1].dst == q.src - p[np - 1].src) p[np - 1].bytes = (size_t)(q.src - p[np - 1].src) + q.bytes;
            else p[np++] = q;
        }
        for (int i = 0; i < np; ++i) HIP_TRY(hipMemcpyAsync(p[i].dst, p[i].src, p[i].bytes, hipMemcpyDeviceToHost, e->stream));
    }
    if (sync) HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

void norm_set_drop(adc_engine *e, NormSet &s);      // (parts/mlp_core.inc, the head of the lifetime chain)

}  // namespace

ADC_EXPORT int adc_abi_version(void) { return ADC_ABI_VERSION; }
ADC_EXPORT int adc_stream_revision(void) { return ADC_STREAM_REVISION; }
ADC_EXPORT const char *adc_last_error(void) { return g_err.c_str(); }

ADC_EXPORT int adc_device_count(int *count)
{
    if (!count) return fail(ADC_EINVAL, "count is NULL");
    int n = 0;
    hipError_t err = hipGetDeviceCount(&n);
    if (err != hipSuccess) { *count = 0; return fail(ADC_EHIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(err)); }
    *count = n;
    return ADC_OK;
}

ADC_EXPORT void adc_engine_destroy(adc_engine *e)
{
    if (!e) return;
    (void)hipSetDevice(e->cfg.device_id);
    for (hipStream_t gs : e->gstream) if (gs) (void)hipStreamSynchronize(gs);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->comm) (void)comm_release(e);
    for (hipStream_t gs : e->gstream) if (gs) (void)hipStreamDestroy(gs);
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    for (hipEvent_t ev : e->ev_join) if (ev) (void)hipEventDestroy(ev);
    for (auto ev : e->ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : e->comm_ev) if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : e->region_ev) if (ev) (void)hipEventDestroy(ev);
    for (void *p : e->allocs) (void)hipFree(p);
    if (e->h_out_block) (void)hipHostFree(e->h_out_block);
    if (e->h_act_block) (void)hipHostFree(e->h_act_block);
    if (e->h_listing) (void)hipHostFree(e->h_listing);
    if (e->h_binding) (void)hipHostFree(e->h_binding);
    if (e->h_direct) (void)hipHostFree(e->h_direct);
    for (void *p : e->curve_allocs) (void)hipFree(p);
    for (void *p : e->mlp_allocs) (void)hipFree(p);
    for (void *p : e->pop_allocs) (void)hipFree(p);
    for (void *p : e->lrn_allocs) (void)hipFree(p);
    for (void *p : e->es_allocs) (void)hipFree(p);
    for (void *p : e->ro_allocs) (void)hipFree(p);
    for (void *p : e->teach_allocs) (void)hipFree(p);
    for (void *p : e->pg_allocs) (void)hipFree(p);
    if (e->pq_host) (void)hipHostFree(e->pq_host);
    for (void *p : e->td3_allocs) (void)hipFree(p);
    for (NormSet *s : {&e->on, &e->rn, &e->tn, &e->sn}) norm_set_drop(e, *s);
    if (e->day_graph) (void)hipGraphExecDestroy(e->day_graph);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

ADC_EXPORT int adc_engine_create(const adc_config *cfg, adc_engine **out)
{
    if (!cfg || !out) return fail(ADC_EINVAL, "cfg/out is NULL");
    *out = nullptr;
    if (cfg->struct_size != sizeof(adc_config)) return fail(ADC_EINVAL, "adc_config.struct_size mismatch (ABI)");
    if (cfg->num_envs <= 0 || cfg->num_keywords <= 0) return fail(ADC_EINVAL, "num_envs and num_keywords must be positive");
    if (cfg->model != ADC_MODEL_IMPLICIT && cfg->model != ADC_MODEL_EXPLICIT && cfg->model != ADC_MODEL_IMPLICIT_GENERAL) return fail(ADC_EINVAL, "unknown model");
    if ((int64_t)cfg->num_envs * cfg->num_keywords > ((int64_t)1 << 31) - 1) return fail(ADC_EINVAL, "num_envs*num_keywords exceeds 2^31-1 per device");
    if ((size_t)cfg->num_keywords * 40 > 160 * 1024) return fail(ADC_EINVAL, "num_keywords > 4096 is not supported");
    int ndev = 0;
    hipError_t err = hipGetDeviceCount(&ndev);
    if (err != hipSuccess || ndev <= 0)
        return fail(ADC_EHIP, "no usable HIP device: this engine has no CPU path (hipGetDeviceCount: " +
                                  std::string(err == hipSuccess ? "0 devices" : hipGetErrorString(err)) + ")");
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(ADC_EINVAL, "device_id out of range");
    HIP_TRY(hipSetDevice(cfg->device_id));
    adc_engine *e = new (std::nothrow) adc_engine();
    if (!e) return fail(ADC_ENOMEM, "host allocation failed");
    e->cfg = *cfg;
    int rc = ADC_OK;
    auto bail = [&](int code) { adc_engine_destroy(e); return code; };
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) return bail(fail(ADC_EHIP, "hipStreamCreate failed"));
    View &v = e->v;
    std::memset(&v, 0, sizeof(v));
    v.N = v.NP = cfg->num_envs; v.K = cfg->num_keywords; v.model = cfg->model; v.max_days = cfg->max_days;
    v.loss_threshold = cfg->loss_threshold;
    v.drift_vol = cfg->drift_vol; v.drift_ctr = cfg->drift_ctr; v.drift_cvr = cfg->drift_cvr;
    v.drift_on = cfg->drift_enabled ? 1 : 0;
    v.imp_thresh = cfg->impression_thresh;
    v.auto_reset = cfg->auto_reset ? 1 : 0;
    v.max_bidders = 30; v.participation_rate = 0.6f; v.num_winners = 1;       // synthetic_kw_classes.py:659-665, :623
    const size_t N = v.N, K = v.K, NK = N * K;
#define A(ptr, count) if ((rc = dev_alloc(e, &(ptr), (count))) != ADC_OK) return bail(rc)
    A(v.params, ADC_P_COUNT * NK);
    A(v.key, N); A(v.tick, N); A(v.day, N); A(v.cum_cents, N); A(v.cum, N); A(v.drift_pending, N); A(v.exact_hint, N);
    A(v.flag_list, N); A(v.xover_list, N); A(v.retry_list, N);
    A(e->d_counters, kCounterInts * (1 + kMaxGroups));
    point_counters(v, e->d_counters);
    A(v.env_cost, N); A(v.env_profit, N); A(v.flags_seen, 3);
    {   // IMPLICIT_GENERAL, a handful of envs: k_step_general_small (ADCRAFT_GENERAL_SMALL=0 / 1 forces either pass: tests)
        bool small = v.model == ADC_MODEL_IMPLICIT_GENERAL && NK <= (size_t)kGSmallMaxKeywords;
        if (const char *ov = std::getenv("ADCRAFT_GENERAL_SMALL")) small = v.model == ADC_MODEL_IMPLICIT_GENERAL && std::atoi(ov) != 0;
        if (small) { A(v.gs_profit, NK); A(v.gs_spend, NK); }
    }
    if (v.model == ADC_MODEL_IMPLICIT && K <= (size_t)kRestMaxK) {
        // what k_step_exact_rows parks for k_step_rest_of_day
        {
            A(v.rest_state, N); A(v.rest_counts, NK); A(v.rest_cost, NK); A(v.rest_rev, NK);
            // K <= 256: the pass and the walk of the marked cells as two kernels (ADCRAFT_REST_SPLIT=0: one)
            // (a handful of envs: the second launch costs more than wave 0's walk; ADCRAFT_REST_SPLIT=1 / 0 forces either)
            bool split = N >= 1024;
            if (const char *ov = std::getenv("ADCRAFT_REST_SPLIT")) split = std::atoi(ov) != 0;
            // (the table the pass hands over instead of a list - 100 MB at 4096 x 256 - only once a budget binds: ensure_rest_table)
            v.rest_marks_stride = kRestMarks * (int)((K + kRowsBlock - 1) / kRowsBlock);
            if (split) { e->rest_table_count = N * adc::kTimesteps * K + 2; A(v.rest_marks, N * (size_t)v.rest_marks_stride); A(v.rest_nmarks, N); }
            if (split && K <= (size_t)kRowsBlock) {        // envs whose budget runs out within the first cells of the day: parked by k_tail_or_flag at once
                {
                    A(v.direct_budget, N); A(v.direct_list, N); A(v.direct_days, 1);
                    if (hipHostMalloc((void **)&e->h_direct, sizeof(int), hipHostMallocMapped) != hipSuccess) return bail(fail(ADC_ENOMEM, "hipHostMalloc (at-once flag)"));
                    *e->h_direct = 0;
                    if (hipHostGetDevicePointer((void **)&v.direct_flag, e->h_direct, 0) != hipSuccess) return bail(fail(ADC_EHIP, "hipHostGetDevicePointer (at-once flag)"));
                }
            }
            v.rest_marks_cap = v.rest_marks_stride;
            if (const char *ov = std::getenv("ADCRAFT_REST_MARKS")) v.rest_marks_cap = std::max(0, std::min(v.rest_marks_stride, std::atoi(ov)));
            if (hipHostMalloc((void **)&e->h_binding, sizeof(int), hipHostMallocMapped) != hipSuccess) return bail(fail(ADC_ENOMEM, "hipHostMalloc (binding flag)"));
            *e->h_binding = 0;
            if (hipHostGetDevicePointer((void **)&v.binding_flag, e->h_binding, 0) != hipSuccess) return bail(fail(ADC_EHIP, "hipHostGetDevicePointer (binding flag)"));
        }
    }
    if (v.model == ADC_MODEL_IMPLICIT && K <= 256) {
        // lists of clicked wins for k_step_click_walk (binding budgets), one per env and sub-timestep: up to 8 per keyword,
        // 1024 per list (the benchmark's dense configuration lists ~420; what the kernel sorts in LDS).
        // ADCRAFT_CLICK_WALK=0 turns the path off, ADCRAFT_CLICK_CAP sets another capacity (tests)
        size_t cap = std::min<size_t>(kWalkRowCapMax, std::max<size_t>(64, 8 * K));
        bool on = true;
        if (const char *ov = std::getenv("ADCRAFT_CLICK_WALK")) on = std::atoi(ov) != 0;
        if (const char *ov = std::getenv("ADCRAFT_CLICK_CAP")) cap = (size_t)std::max(1, std::min(kWalkRowCapMax, std::atoi(ov)));
        if (on && N * kClickSegments * cap * sizeof(uint2) <= ((size_t)4 << 30)) {
            // (the records themselves - 840 MB at 4096 x 256 - only once an env asks for lists: ensure_click_lists)
            e->click_rec_count = N * kClickSegments * cap;
            A(v.click_count, N * adc::kTimesteps); A(v.click_tick, N);
            A(v.click_row_hint, N); A(v.click_price_hint, N);
            if (hipHostMalloc((void **)&e->h_listing, sizeof(int), hipHostMallocMapped) != hipSuccess) return bail(fail(ADC_ENOMEM, "hipHostMalloc (listing flag)"));
            *e->h_listing = 0;
            if (hipHostGetDevicePointer((void **)&v.listing_flag, e->h_listing, 0) != hipSuccess) return bail(fail(ADC_EHIP, "hipHostGetDevicePointer (listing flag)"));
            v.click_cap = (int)cap;
            v.click_list_max = 4096;        // (measured on the dense benchmark law scaled to lower click rates: tools/exp_binding_ctr.py)
            if (const char *ov = std::getenv("ADCRAFT_CLICK_WALK_MAX")) v.click_list_max = std::max(0, std::atoi(ov));
        }
    }
    {
        // the ten step outputs as slices of one block (16-byte aligned each), in adc_step_out order
        const size_t sizes[10] = {NK * 4, NK * 4, NK * 4, NK * 4, NK * 4, N * 8, N * 8, N * 4, N, N};
        size_t off = 0;
        for (int i = 0; i < 10; ++i) { e->out_off[i] = off; off += (sizes[i] + 15) & ~(size_t)15; }
        e->out_block_bytes = off;
        A(e->d_out_block, off);
        unsigned char *b = e->d_out_block;
        v.imp = (int32_t *)(b + e->out_off[0]); v.clk = (int32_t *)(b + e->out_off[1]); v.conv = (int32_t *)(b + e->out_off[2]);
        v.cost = (float *)(b + e->out_off[3]); v.rev = (float *)(b + e->out_off[4]);
        v.reward = (double *)(b + e->out_off[5]); v.cum_profit = (double *)(b + e->out_off[6]);
        v.day_out = (int32_t *)(b + e->out_off[7]); v.term = b + e->out_off[8]; v.trunc = b + e->out_off[9];
        A(e->d_bids, NK + N);                        // bids, then the budgets
        e->d_budget = e->d_bids + NK;
        if (off <= kSmallBlockBytes) {               // page-locked mirrors only where one copy beats ten
            if (hipHostMalloc((void **)&e->h_out_block, off, hipHostMallocDefault) != hipSuccess) e->h_out_block = nullptr;
            if (hipHostMalloc((void **)&e->h_act_block, (NK + N) * 4, hipHostMallocDefault) != hipSuccess) e->h_act_block = nullptr;
        }
    }
    A(v.metric_profit, K); A(v.metric_scalars, 8); A(v.metric_env, 4 * N); A(v.metric_lo, NK); A(v.metric_hi, NK);
#undef A
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cfg->device_id) == hipSuccess && prop.multiProcessorCount > 0) e->num_cus = prop.multiProcessorCount;
    }
    if (const char *ov = std::getenv("ADCRAFT_FAST_TILE_KW")) { const int t = std::atoi(ov); if (t >= 16 && t <= 256 && (t & (t - 1)) == 0) e->fast_tile_kw = t; }
    if (const char *ov = std::getenv("ADCRAFT_IDEAL_FULL_SCAN")) e->ideal_full_scan = std::atoi(ov) != 0;
    if (const char *ov = std::getenv("ADCRAFT_FAIL_LAZY_ALLOC")) e->fail_lazy_alloc = std::atoi(ov) != 0;
    if (const char *ov = std::getenv("ADCRAFT_STREAM_GROUPS")) e->groups_override = std::max(0, std::min(kMaxGroups, std::atoi(ov)));
    if (const char *ov = std::getenv("ADCRAFT_FAST_TILES_PER_WG")) e->fast_tiles_per_wg = std::max(0, std::atoi(ov));
    if (const char *ov = std::getenv("ADCRAFT_FAST_VARIANT")) e->fast_variant = std::max(0, std::min(2, std::atoi(ov)));
    hipLaunchKernelGGL(k_build_log_table, dim3((adc::kNormTableEntries + 256) / 256), dim3(256), 0, e->stream);
    hipLaunchKernelGGL(k_init_keys, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, e->stream, v, cfg->seed, cfg->env_id_base);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess)
        return bail(fail(ADC_EHIP, "engine initialisation kernel failed (is this a gfx950 device?)"));
    *out = e;
    return ADC_OK;
}

// (every entry point but adc_engine_step_device may enqueue work on the engine's stream that the env groups' next step has to see:
//  launch_step then makes the groups' streams wait for the engine's - needs_fork)
#define ENGINE_GUARD(e)                                                   \
    if (!(e)) return fail(ADC_EINVAL, "engine handle is NULL");           \
    (e)->needs_fork = true;                                               \
    (e)->api_since_step = true;                                           \
    HIP_TRY(hipSetDevice((e)->cfg.device_id));                            \
    { const int join_rc_ = join_groups(e); if (join_rc_) return join_rc_; } (void)0
#define ENGINE_GUARD_STEP(e)                                              \
    if (!(e)) return fail(ADC_EINVAL, "engine handle is NULL");           \
    HIP_TRY(hipSetDevice((e)->cfg.device_id))

namespace {
// Device-side work BETWEEN two steps of a chain that touches every env on its own - the agent's update + act, the per-step ideal,
// the oracle bidder, the engine's own action sampler: while the chain's last step ran as env groups it is launched group by group
// on the groups' streams, behind that group's step and in front of its next one, and nothing is forked or joined (four engines of
// a quarter of the envs side by side measured the closed loop - agent, ideal, step - at 0.237 ms per day against 0.431 for one
// engine: the ideal kernel is a latency-bound search that leaves the chip to the other groups' step kernels).  Outside a chain -
// the caller asked for something else since the last step, the last step was one group, the stream is exposed, a capture or a
// profile is running - it goes on the engine's stream as ever.  Either way it does not end a chain (api_since_step stays).
// launch(view, policy view, stream, bids of the view's first env, budgets of the view's first env)
template <class Launch>
int launch_chained(adc_engine *e, Launch launch)
{
    const int G = e->last_groups;
    const bool grouped = G > 1 && !e->api_since_step && !e->stream_exposed && !e->in_capture && !e->profiling;
    if (!grouped) {
        { const int rc = join_groups(e); if (rc) return rc; }
        e->needs_fork = true;
        launch(e->v, e->pol, e->stream, e->d_bids, e->d_budget);
        HIP_TRY(hipGetLastError());
        return ADC_OK;
    }
    if (e->needs_fork) {
        HIP_TRY(hipEventRecord(e->ev_fork, e->stream));
        for (int g = 0; g < G; ++g) HIP_TRY(hipStreamWaitEvent(e->gstream[g], e->ev_fork, 0));
        e->needs_fork = false;
    }
    for (int g = 0; g < G; ++g) {
        int e0 = 0;
        const View vg = group_view(e, g, G, &e0);
        const PolicyView pg = policy_group_view(e, g, G);
        launch(vg, pg, e->gstream[g], e->d_bids + (size_t)e0 * e->v.K, e->d_budget + e0);
        HIP_TRY(hipGetLastError());
    }
    e->groups_pending = true;
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_step_device(adc_engine *e, const float *d_bids_nk, const float *d_budget_n)
{
    ENGINE_GUARD_STEP(e);
    if (d_bids_nk || d_budget_n) e->needs_fork = e->api_since_step = true;       // (the caller's own buffers: ordered against the engine's stream by the caller)
    if (!e->have_reset) return fail(ADC_ESTATE, "reset required, need to generate keywords to bid on");
    return launch_step(e, d_bids_nk ? d_bids_nk : e->d_bids, d_budget_n ? d_budget_n : e->d_budget, nullptr, /* lazy_join = */ true);
}

ADC_EXPORT int adc_engine_out_offsets(const adc_engine *e, size_t offsets[10], size_t *block_bytes)
{
    if (!e || !offsets) return fail(ADC_EINVAL, "null argument");
    for (int i = 0; i < 10; ++i) offsets[i] = e->out_off[i];
    if (block_bytes) *block_bytes = e->out_block_bytes;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_fetch(adc_engine *e, adc_step_out *out)
{
    ENGINE_GUARD(e);
    return fetch(e, out);
}

ADC_EXPORT int adc_engine_synchronize(adc_engine *e)
{
    ENGINE_GUARD(e);
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_step(adc_engine *e, const float *bids_nk, const float *budget_n, adc_step_out *out)
{
    ENGINE_GUARD(e);
    if (!e->have_reset) return fail(ADC_ESTATE, "reset required, need to generate keywords to bid on");
    if (!bids_nk || !budget_n) return fail(ADC_EINVAL, "bids/budget is NULL");
    const size_t NK = (size_t)e->v.N * e->v.K;
    if (e->h_act_block) {
        std::memcpy(e->h_act_block, bids_nk, NK * 4);
        std::memcpy(e->h_act_block + NK, budget_n, (size_t)e->v.N * 4);
        HIP_TRY(hipMemcpyAsync(e->d_bids, e->h_act_block, (NK + e->v.N) * 4, hipMemcpyHostToDevice, e->stream));
    } else {
        HIP_TRY(hipMemcpyAsync(e->d_bids, bids_nk, NK * 4, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(e->d_budget, budget_n, (size_t)e->v.N * 4, hipMemcpyHostToDevice, e->stream));
    }
    int rc = launch_step(e, e->d_bids, e->d_budget, nullptr);
    if (rc) return rc;
    return fetch(e, out);
}

// The same step without waiting for it: actions up, kernels, outputs down are enqueued on the engine's stream and the call
// returns.  With page-locked host buffers (adc_host_alloc) the copies are true DMA transfers that overlap the kernels and
// copies of OTHER engines on the device - which is how a vector env split into a few engines hides most of the PCIe time of
// a synchronous step (adcraft_amd/vector_env.py).  The buffers must stay untouched until adc_engine_wait returns.
ADC_EXPORT int adc_engine_step_async(adc_engine *e, const float *bids_nk, const float *budget_n, adc_step_out *out)
{
    ENGINE_GUARD(e);
    if (!e->have_reset) return fail(ADC_ESTATE, "reset required, need to generate keywords to bid on");
    if (!bids_nk || !budget_n) return fail(ADC_EINVAL, "bids/budget is NULL");
    const size_t NK = (size_t)e->v.N * e->v.K;
    HIP_TRY(hipMemcpyAsync(e->d_bids, bids_nk, NK * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_budget, budget_n, (size_t)e->v.N * 4, hipMemcpyHostToDevice, e->stream));
    int rc = launch_step(e, e->d_bids, e->d_budget, nullptr);
    if (rc) return rc;
    return fetch(e, out, false);
}

ADC_EXPORT int adc_engine_step_flat_async(adc_engine *e, const float *flat_actions, float *flat_obs, double *reward, uint8_t *terminated,
                                          uint8_t *truncated)
{
    ENGINE_GUARD(e);
    if (!e->have_reset) return fail(ADC_ESTATE, "reset required, need to generate keywords to bid on");
    if (!flat_actions || !flat_obs) return fail(ADC_EINVAL, "flat_actions/flat_obs is NULL");
    const size_t N = e->v.N, K = e->v.K;
    if (!e->d_flat_obs) { int rc = dev_alloc(e, &e->d_flat_obs, N * (5 * K + 2)); if (rc) return rc; }
    if (!e->d_flat_actions) { int rc = dev_alloc(e, &e->d_flat_actions, N * (K + 1)); if (rc) return rc; }
    float *const keep = e->v.flat_obs;
    e->v.flat_obs = e->d_flat_obs;
    HIP_TRY(hipMemcpyAsync(e->d_flat_actions, flat_actions, N * (K + 1) * 4, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_unflatten_actions, dim3((unsigned)((K + 255) / 256), (unsigned)N), dim3(256), 0, e->stream, e->v,
                       e->d_flat_actions, e->d_bids, e->d_budget);
    int rc = hipGetLastError() == hipSuccess ? launch_step(e, e->d_bids, e->d_budget, nullptr) : fail(ADC_EHIP, "k_unflatten_actions launch failed");
    e->v.flat_obs = keep;
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(flat_obs, e->d_flat_obs, N * (5 * K + 2) * 4, hipMemcpyDeviceToHost, e->stream));
    if (reward) HIP_TRY(hipMemcpyAsync(reward, e->v.reward, N * 8, hipMemcpyDeviceToHost, e->stream));
    if (terminated) HIP_TRY(hipMemcpyAsync(terminated, e->v.term, N, hipMemcpyDeviceToHost, e->stream));
    if (truncated) HIP_TRY(hipMemcpyAsync(truncated, e->v.trunc, N, hipMemcpyDeviceToHost, e->stream));
    return ADC_OK;
}

// completes everything enqueued on the engine's stream (the asynchronous steps above)
ADC_EXPORT int adc_engine_wait(adc_engine *e)
{
    ENGINE_GUARD(e);
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_step_flat(adc_engine *e, const float *flat_actions, float *flat_obs, double *reward, uint8_t *terminated,
                                    uint8_t *truncated)
{
    ENGINE_GUARD(e);
    if (!e->have_reset) return fail(ADC_ESTATE, "reset required, need to generate keywords to bid on");
    if (!flat_actions || !flat_obs) return fail(ADC_EINVAL, "flat_actions/flat_obs is NULL");
    const size_t N = e->v.N, K = e->v.K;
    if (!e->d_flat_obs) {
        int rc = dev_alloc(e, &e->d_flat_obs, N * (5 * K + 2));
        if (rc) return rc;
    }
    if (!e->d_flat_actions) {
        int rc = dev_alloc(e, &e->d_flat_actions, N * (K + 1));
        if (rc) return rc;
    }
    float *const keep = e->v.flat_obs;
    e->v.flat_obs = e->d_flat_obs;                     // flatten after this step even if not enabled permanently
    HIP_TRY(hipMemcpyAsync(e->d_flat_actions, flat_actions, N * (K + 1) * 4, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_unflatten_actions, dim3((unsigned)((K + 255) / 256), (unsigned)N), dim3(256), 0, e->stream, e->v,
                       e->d_flat_actions, e->d_bids, e->d_budget);
    int rc = hipGetLastError() == hipSuccess ? launch_step(e, e->d_bids, e->d_budget, nullptr) : fail(ADC_EHIP, "k_unflatten_actions launch failed");
    e->v.flat_obs = keep;
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(flat_obs, e->d_flat_obs, N * (5 * K + 2) * 4, hipMemcpyDeviceToHost, e->stream));
    if (reward) HIP_TRY(hipMemcpyAsync(reward, e->v.reward, N * 8, hipMemcpyDeviceToHost, e->stream));
    if (terminated) HIP_TRY(hipMemcpyAsync(terminated, e->v.term, N, hipMemcpyDeviceToHost, e->stream));
    if (truncated) HIP_TRY(hipMemcpyAsync(truncated, e->v.trunc, N, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}
