// host_api.inc - engine object and the extern "C" entry points of include/adcraft_engine.h
// (part of the single translation unit adc_engine.hip; see that file for the overview)
// -------------------------------------------------------------------------------------------------
// host side
// -------------------------------------------------------------------------------------------------
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

ADC_EXPORT int adc_engine_set_params(adc_engine *e, int param_id, const float *host_nk)
{
    ENGINE_GUARD(e);
    if (param_id < 0 || param_id >= ADC_P_COUNT || !host_nk) return fail(ADC_EINVAL, "bad param_id or NULL buffer");
    const size_t NK = (size_t)e->v.N * e->v.K;
    HIP_TRY(hipMemcpyAsync(e->v.params + (size_t)param_id * NK, host_nk, NK * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (param_id == ADC_P_VOL_MEAN) e->volume_hint_dirty = true;
    forget_replayable_steps(e);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_get_params(adc_engine *e, int param_id, float *host_nk)
{
    ENGINE_GUARD(e);
    if (param_id < 0 || param_id >= ADC_P_COUNT || !host_nk) return fail(ADC_EINVAL, "bad param_id or NULL buffer");
    const size_t NK = (size_t)e->v.N * e->v.K;
    if (e->v.drift_on) {
        materialize_drift(e);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(host_nk, e->v.params + (size_t)param_id * NK, NK * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_set_env_params(adc_engine *e, int env, const float *host_8k)
{
    ENGINE_GUARD(e);
    if (env < 0 || env >= e->v.N || !host_8k) return fail(ADC_EINVAL, "env out of range or NULL buffer");
    const size_t K = e->v.K, NK = (size_t)e->v.N * K;
    for (int p = 0; p < ADC_P_COUNT; ++p)
        HIP_TRY(hipMemcpyAsync(e->v.params + p * NK + env * K, host_8k + p * K, K * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->volume_hint_dirty = true;
    forget_replayable_steps(e);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_generate_keywords(adc_engine *e, const adc_quantiles *q, float no_vol_prob, uint32_t serial,
                                            const uint8_t *env_mask)
{
    ENGINE_GUARD(e);
    if (e->v.model != ADC_MODEL_IMPLICIT) return fail(ADC_EINVAL, "device keyword generation is provided for IMPLICIT keywords");
    if (!q) return fail(ADC_EINVAL, "quantile tables are NULL");
    std::vector<void *> tmp;
    auto cleanup = [&]() { for (void *p : tmp) (void)hipFree(p); };
    KeygenTables tabs;
    for (int i = 0; i < 7; ++i) {
        const int B = q->buckets[i];
        if (B <= 0 || !q->mins[i] || !q->medians[i] || !q->maxs[i]) { cleanup(); return fail(ADC_EINVAL, "every quantity needs at least one bucket"); }
        float *d = nullptr;
        if (hipMalloc((void **)&d, (size_t)B * 12) != hipSuccess) { cleanup(); return fail(ADC_ENOMEM, "hipMalloc (quantiles) failed"); }
        tmp.push_back(d);
        if (hipMemcpyAsync(d, q->mins[i], (size_t)B * 4, hipMemcpyHostToDevice, e->stream) != hipSuccess ||
            hipMemcpyAsync(d + B, q->medians[i], (size_t)B * 4, hipMemcpyHostToDevice, e->stream) != hipSuccess ||
            hipMemcpyAsync(d + 2 * B, q->maxs[i], (size_t)B * 4, hipMemcpyHostToDevice, e->stream) != hipSuccess) { cleanup(); return fail(ADC_EHIP, "quantile upload failed"); }
        tabs.t[i] = adc::QuantileTable{d, d + B, d + 2 * B, B};
    }
    uint8_t *d_mask = nullptr;
    if (env_mask) {
        if (hipMalloc((void **)&d_mask, (size_t)e->v.N) != hipSuccess) { cleanup(); return fail(ADC_ENOMEM, "hipMalloc (mask) failed"); }
        tmp.push_back(d_mask);
        if (hipMemcpyAsync(d_mask, env_mask, (size_t)e->v.N, hipMemcpyHostToDevice, e->stream) != hipSuccess) { cleanup(); return fail(ADC_EHIP, "mask upload failed"); }
    }
    hipLaunchKernelGGL(k_generate_keywords, dim3((unsigned)((e->v.K + 255) / 256), (unsigned)e->v.N), dim3(256), 0, e->stream, e->v, tabs,
                       no_vol_prob, serial, d_mask);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    cleanup();
    HIP_TRY(err);
    e->volume_hint_dirty = true;
    forget_replayable_steps(e);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_generate_explicit_keywords(adc_engine *e, uint32_t serial, const uint8_t *env_mask)
{
    ENGINE_GUARD(e);
    if (e->v.model != ADC_MODEL_EXPLICIT) return fail(ADC_EINVAL, "sample_random_keywords' law is the EXPLICIT model's (IMPLICIT keywords: adc_engine_generate_keywords)");
    uint8_t *d_mask = nullptr;
    if (env_mask) {
        if (hipMalloc((void **)&d_mask, (size_t)e->v.N) != hipSuccess) { (void)hipGetLastError(); return fail(ADC_ENOMEM, "hipMalloc (mask) failed"); }
        if (hipMemcpyAsync(d_mask, env_mask, (size_t)e->v.N, hipMemcpyHostToDevice, e->stream) != hipSuccess) { (void)hipFree(d_mask); return fail(ADC_EHIP, "mask upload failed"); }
    }
    hipLaunchKernelGGL(k_generate_explicit_keywords, dim3((unsigned)((e->v.K + 255) / 256), (unsigned)e->v.N), dim3(256), 0, e->stream, e->v, serial, d_mask);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (d_mask) (void)hipFree(d_mask);
    HIP_TRY(err);
    e->volume_hint_dirty = true;
    forget_replayable_steps(e);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_reset(adc_engine *e, const uint8_t *env_mask, const uint64_t *seeds)
{
    ENGINE_GUARD(e);
    const size_t N = e->v.N;
    uint8_t *d_mask = nullptr;
    uint64_t *d_seeds = nullptr;
    if (env_mask) { HIP_TRY(hipMalloc((void **)&d_mask, N)); HIP_TRY(hipMemcpyAsync(d_mask, env_mask, N, hipMemcpyHostToDevice, e->stream)); }
    if (seeds) { HIP_TRY(hipMalloc((void **)&d_seeds, N * 8)); HIP_TRY(hipMemcpyAsync(d_seeds, seeds, N * 8, hipMemcpyHostToDevice, e->stream)); }
    hipLaunchKernelGGL(k_reset, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, e->stream, e->v, d_mask, d_seeds);
    hipError_t err = hipGetLastError();
    // the observation reset() returns is all zeros (gymnasium_kw_env.py:329-344): device-resident callers read it
    if (err == hipSuccess) {
        hipLaunchKernelGGL(k_clear_obs, dim3((unsigned)((e->v.K + 255) / 256), (unsigned)N), dim3(256), 0, e->stream, e->v, d_mask);
        err = hipGetLastError();
    }
    // (a reset env's running discounted return ends with its episode, the PPO / A2C learners', the TD3 learners' and the SAC
    //  learners'; nothing is enqueued without a reward normaliser)
    for (const NormSet *s : {&e->rn, &e->tn, &e->sn}) {
        if (err != hipSuccess || !s->rew.G) continue;
        hipLaunchKernelGGL(k_rew_norm_carry_reset, dim3((unsigned)((N + kRewNormBlock - 1) / kRewNormBlock)), dim3(kRewNormBlock), 0, e->stream, (int)N, d_mask,
                           s->rew.G);
        err = hipGetLastError();
    }
    // (... and so does its observation history; nothing is enqueued without one)
    if (err == hipSuccess && e->have_mlp && e->mp.hist) {
        hipLaunchKernelGGL(k_mlp_hist_forget, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, e->stream, (int)N, d_mask, e->mp.last);
        err = hipGetLastError();
    }
    hipError_t err2 = hipStreamSynchronize(e->stream);
    if (d_mask) (void)hipFree(d_mask);
    if (d_seeds) (void)hipFree(d_seeds);
    HIP_TRY(err);
    HIP_TRY(err2);
    e->have_reset = true;
    e->last_step = 0;
    e->stream_steps = 0;
    e->env_moves += 1;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_set_limits(adc_engine *e, int32_t max_days, double loss_threshold)
{
    ENGINE_GUARD(e);
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->v.max_days = max_days;
    e->v.loss_threshold = loss_threshold;
    e->cfg.max_days = max_days;
    e->cfg.loss_threshold = loss_threshold;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_set_drift(adc_engine *e, int32_t enabled, float drift_vol, float drift_ctr, float drift_cvr)
{
    ENGINE_GUARD(e);
    if (!enabled && e->v.drift_on) {      // apply what is pending under the old setting, then switch off
        materialize_drift(e);
        HIP_TRY(hipGetLastError());
        forget_replayable_steps(e);       // (the parameters have moved, and with drift off nothing would say so any more)
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->v.drift_on = enabled ? 1 : 0;
    e->v.drift_vol = drift_vol; e->v.drift_ctr = drift_ctr; e->v.drift_cvr = drift_cvr;
    if (!enabled) HIP_TRY(hipMemsetAsync(e->v.drift_pending, 0, (size_t)e->v.N, e->stream));
    return ADC_OK;
}

namespace {
// what adc_engine_set_drift_mask / adc_engine_set_env_drift do before they swap: the pending update_keywords() of every env is
// the one the previous step scheduled, so it moves the planes under the selection and magnitudes in force when it was
// scheduled; then nothing in flight reads the old device copy when it is overwritten
int settle_pending_drift(adc_engine *e)
{
    if (e->v.drift_on) {
        materialize_drift(e);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_set_drift_mask(adc_engine *e, const uint8_t *mask_nk)
{
    ENGINE_GUARD(e);
    { const int rc = settle_pending_drift(e); if (rc) return rc; }
    if (!mask_nk) { e->v.drift_bits = nullptr; return ADC_OK; }
    const size_t N = (size_t)e->v.N, K = (size_t)e->v.K, W = (K + 31) / 32;
    std::vector<uint32_t> bits(N * W, 0u);
    for (size_t n = 0; n < N; ++n)
        for (size_t k = 0; k < K; ++k)
            if (mask_nk[n * K + k]) bits[n * W + k / 32] |= 1u << (k % 32);
    if (!e->d_drift_bits) { const int rc = dev_alloc(e, &e->d_drift_bits, N * W); if (rc) return rc; }
    HIP_TRY(hipMemcpyAsync(e->d_drift_bits, bits.data(), N * W * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->v.drift_bits = e->d_drift_bits;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_set_env_drift(adc_engine *e, const float *rates_n3)
{
    ENGINE_GUARD(e);
    { const int rc = settle_pending_drift(e); if (rc) return rc; }
    if (!rates_n3) { e->v.drift_rate = nullptr; return ADC_OK; }
    const size_t N = (size_t)e->v.N;
    if (!e->d_drift_rate) { const int rc = dev_alloc(e, &e->d_drift_rate, N * 3); if (rc) return rc; }
    HIP_TRY(hipMemcpyAsync(e->d_drift_rate, rates_n3, N * 3 * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->v.drift_rate = e->d_drift_rate;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_get_rng_state(adc_engine *e, uint64_t *keys_n, uint32_t *ticks_n)
{
    ENGINE_GUARD(e);
    const size_t N = e->v.N;
    if (keys_n) HIP_TRY(hipMemcpyAsync(keys_n, e->v.key, N * 8, hipMemcpyDeviceToHost, e->stream));
    if (ticks_n) HIP_TRY(hipMemcpyAsync(ticks_n, e->v.tick, N * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_set_rng_state(adc_engine *e, const uint64_t *keys_n, const uint32_t *ticks_n)
{
    ENGINE_GUARD(e);
    const size_t N = e->v.N;
    if (keys_n) HIP_TRY(hipMemcpyAsync(e->v.key, keys_n, N * 8, hipMemcpyHostToDevice, e->stream));
    if (ticks_n) HIP_TRY(hipMemcpyAsync(e->v.tick, ticks_n, N * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    forget_replayable_steps(e);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_get_episode_state(adc_engine *e, int32_t *day_n, double *cum_profit_n)
{
    ENGINE_GUARD(e);
    const size_t N = e->v.N;
    if (day_n) HIP_TRY(hipMemcpyAsync(day_n, e->v.day, N * 4, hipMemcpyDeviceToHost, e->stream));
    if (cum_profit_n) {
        if (e->v.model == ADC_MODEL_IMPLICIT) {
            std::vector<int64_t> c(N);
            HIP_TRY(hipMemcpyAsync(c.data(), e->v.cum_cents, N * 8, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            for (size_t i = 0; i < N; ++i) cum_profit_n[i] = (double)c[i] / 100.0;
        } else {
            HIP_TRY(hipMemcpyAsync(cum_profit_n, e->v.cum, N * 8, hipMemcpyDeviceToHost, e->stream));
        }
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_set_episode_state(adc_engine *e, const int32_t *day_n, const double *cum_profit_n)
{
    ENGINE_GUARD(e);
    const size_t N = e->v.N;
    if (day_n) HIP_TRY(hipMemcpyAsync(e->v.day, day_n, N * 4, hipMemcpyHostToDevice, e->stream));
    if (cum_profit_n) {
        std::vector<int64_t> c(N);
        for (size_t i = 0; i < N; ++i) c[i] = (int64_t)std::llrint(cum_profit_n[i] * 100.0);
        HIP_TRY(hipMemcpyAsync(e->v.cum_cents, c.data(), N * 8, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(e->v.cum, cum_profit_n, N * 8, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->have_reset = true;
    e->last_step = 0;
    e->stream_steps = 0;
    e->env_moves += 1;
    return ADC_OK;
}

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
    if (hipMalloc((void **)&d, b_rec + b_cost + b_bids + b_share + 16) != hipSuccess) return fail(ADC_ENOMEM, "hipMalloc failed");
    auto done = [&](int code) { (void)hipFree(d); return code; };
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
        return done(fail(ADC_EHIP, "upload failed"));
    TapeView none{};
#define WALK(MODEL) \
    if (tape) hipLaunchKernelGGL((k_step_exact<MODEL, true>), dim3(1), dim3(kWave), lds, e->stream, v, d_bids, e->d_budget, *tape, 0, rp); \
    else hipLaunchKernelGGL((k_step_exact<MODEL, false>), dim3(1), dim3(kWave), lds, e->stream, v, d_bids, e->d_budget, none, 0, rp)
    if (v.model == ADC_MODEL_IMPLICIT) { WALK(ADC_MODEL_IMPLICIT); }
    else if (v.model == ADC_MODEL_IMPLICIT_GENERAL) { WALK(ADC_MODEL_IMPLICIT_GENERAL); }
    else { WALK(ADC_MODEL_EXPLICIT); }
#undef WALK
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) return done(fail(ADC_EHIP, "replay kernel failed"));
    int n = 0;
    if (hipMemcpy(&n, rp.count, 4, hipMemcpyDeviceToHost) != hipSuccess) return done(fail(ADC_EHIP, "download failed"));
    *count = n;
    const size_t m = std::min<size_t>((size_t)std::max(n, 0), cap);
    if (m) {
        std::vector<int4> rec(m);
        if (hipMemcpy(rec.data(), rp.records, m * sizeof(int4), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(cost, rp.costs, m * 8, hipMemcpyDeviceToHost) != hipSuccess)
            return done(fail(ADC_EHIP, "download failed"));
        for (size_t i = 0; i < m; ++i) {
            keyword[i] = rec[i].x;
            timestep[i] = rec[i].y;
            revenue[i] = rec[i].z < 0 ? -1.0 : (double)rec[i].z / 100.0;
        }
    }
    if (share_volume_k && hipMemcpy(share_volume_k, rp.share_volume, b_share, hipMemcpyDeviceToHost) != hipSuccess) return done(fail(ADC_EHIP, "download failed"));
    return done(ADC_OK);
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

// a host adc_tape on the device (adc_engine_step_replay, adc_engine_outcomes_replay_tape); the copies live as long as the object
struct TapeUpload {
    adc_engine *e;
    std::vector<void *> tmp;
    TapeView tv{};
    int64_t *d_end = nullptr;
    explicit TapeUpload(adc_engine *engine) : e(engine) {}
    ~TapeUpload() { for (void *p : tmp) (void)hipFree(p); }
    int up(const void *host, size_t bytes, const void **dev)
    {
        *dev = nullptr;
        if (!host) return ADC_OK;
        void *q = nullptr;
        if (hipMalloc(&q, bytes ? bytes : 8) != hipSuccess) return fail(ADC_ENOMEM, "hipMalloc (tape) failed");
        tmp.push_back(q);
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
        if (!rc && hipMalloc((void **)&d_end, 6 * N * 8 + 8) != hipSuccess) rc = fail(ADC_ENOMEM, "hipMalloc (tape cursors) failed");
        if (rc) return rc;
        tmp.push_back(d_end);
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
    if (!rc) rc = t.check_exhausted();
    if (!rc) {
        int64_t *dst[6] = {tape->end_bid, tape->end_ximp, tape->end_xcost, tape->end_click, tape->end_conv, tape->end_rev};
        for (int i = 0; i < 6 && !rc; ++i)
            if (dst[i] && hipMemcpy(dst[i], t.d_end + i * N, N * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(ADC_EHIP, "cursor download failed");
    }
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
    if (!rc) rc = t.check_exhausted();
    return rc;
}

ADC_EXPORT int adc_engine_set_general_model(adc_engine *e, int32_t max_bidders, float participation_rate, int32_t num_winners)
{
    ENGINE_GUARD(e);
    if (max_bidders < 0 || max_bidders > 252 || (num_winners != 1 && num_winners != 2)) return fail(ADC_EINVAL, "max_bidders must be in [0, 252] and num_winners 1 or 2");
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->v.max_bidders = max_bidders;
    e->v.participation_rate = participation_rate;
    e->v.num_winners = num_winners;
    forget_replayable_steps(e);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_update_keywords(adc_engine *e)
{
    ENGINE_GUARD(e);
    if (!e->v.drift_on) return ADC_OK;        // updater_mask is None: no-op (gymnasium_kw_env.py:125-126)
    materialize_drift(e);
    hipLaunchKernelGGL(k_force_drift, dim3(e->v.N), dim3(256), 0, e->stream, e->v);     // (advances every env's tick)
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    forget_replayable_steps(e);
    return ADC_OK;
}

ADC_EXPORT int adc_host_alloc(size_t bytes, void **out)
{
    if (!out) return fail(ADC_EINVAL, "out is NULL");
    *out = nullptr;
    void *p = nullptr;
    hipError_t err = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
    if (err != hipSuccess) return fail(ADC_ENOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(err));
    *out = p;
    return ADC_OK;
}

ADC_EXPORT void adc_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

ADC_EXPORT int adc_engine_device_buffer(adc_engine *e, int buffer_id, void **dptr, size_t *bytes)
{
    ENGINE_GUARD(e);
    if (!dptr) return fail(ADC_EINVAL, "dptr is NULL");
    const View &v = e->v;
    const size_t N = v.N, K = v.K, NK = N * K;
    void *p = nullptr;
    size_t b = 0;
    switch (buffer_id) {
    case ADC_BUF_PARAMS: p = v.params; b = ADC_P_COUNT * NK * 4; break;
    case ADC_BUF_BIDS: p = e->d_bids; b = NK * 4; break;
    case ADC_BUF_BUDGET: p = e->d_budget; b = N * 4; break;
    case ADC_BUF_IMPRESSIONS: p = v.imp; b = NK * 4; break;
    case ADC_BUF_CLICKS: p = v.clk; b = NK * 4; break;
    case ADC_BUF_CONVERSIONS: p = v.conv; b = NK * 4; break;
    case ADC_BUF_COST: p = v.cost; b = NK * 4; break;
    case ADC_BUF_REVENUE: p = v.rev; b = NK * 4; break;
    case ADC_BUF_REWARD: p = v.reward; b = N * 8; break;
    case ADC_BUF_CUM_PROFIT: p = v.cum_profit; b = N * 8; break;
    case ADC_BUF_DAYS: p = v.day_out; b = N * 4; break;
    case ADC_BUF_TERMINATED: p = v.term; b = N; break;
    case ADC_BUF_TRUNCATED: p = v.trunc; b = N; break;
    case ADC_BUF_METRIC_PROFIT: p = v.metric_profit; b = K * 8; break;
    case ADC_BUF_METRIC_SCALARS: p = v.metric_scalars; b = 8 * 8; break;
    case ADC_BUF_FLAT_OBS:
        if (!v.flat_obs) return fail(ADC_ESTATE, "flat observations are not enabled (adc_engine_flat_obs_enable)");
        p = v.flat_obs; b = N * (5 * K + 2) * 4; break;
    case ADC_BUF_ROLLOUT_ACTION: case ADC_BUF_ROLLOUT_LOGP: case ADC_BUF_ROLLOUT_VALUE: case ADC_BUF_ROLLOUT_REWARD:
    case ADC_BUF_ROLLOUT_TERMINATED: case ADC_BUF_ROLLOUT_TRUNCATED: case ADC_BUF_ROLLOUT_OBS: {
        if (e->ro_T == 0) return fail(ADC_ESTATE, "the rollout record is not enabled (adc_engine_rollout_enable)");
        const size_t tn = (size_t)e->ro_T * N;
        if (buffer_id == ADC_BUF_ROLLOUT_ACTION) { p = e->ro_action; b = tn * (size_t)e->mp.A * 4; }
        else if (buffer_id == ADC_BUF_ROLLOUT_LOGP) { p = e->ro_logp; b = tn * 4; }
        else if (buffer_id == ADC_BUF_ROLLOUT_VALUE) { p = e->ro_value; b = tn * 4; }
        else if (buffer_id == ADC_BUF_ROLLOUT_REWARD) { p = e->ro_reward; b = tn * 4; }
        else if (buffer_id == ADC_BUF_ROLLOUT_TERMINATED) { p = e->ro_term; b = tn; }
        else if (buffer_id == ADC_BUF_ROLLOUT_TRUNCATED) { p = e->ro_trunc; b = tn; }
        else {
            if (!e->ro_obs) return fail(ADC_ESTATE, "the record was enabled without ADC_ROLLOUT_OBS");
            p = e->ro_obs; b = tn * (size_t)e->mp.D * 4;
        }
        break;
    }
    default: return fail(ADC_EINVAL, "unknown buffer id");
    }
    *dptr = p;
    if (bytes) *bytes = b;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_set_env_groups(adc_engine *e, int32_t groups)
{
    ENGINE_GUARD(e);
    if (groups < 0 || groups > kMaxGroups) return fail(ADC_EINVAL, "env groups: 0 (the engine chooses) or 1..4");
    e->groups_override = groups;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_env_groups(adc_engine *e, int32_t *groups)
{
    ENGINE_GUARD(e);
    if (!groups) return fail(ADC_EINVAL, "groups is NULL");
    *groups = e->last_groups;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_stream(adc_engine *e, void **hip_stream)
{
    ENGINE_GUARD(e);
    if (!hip_stream) return fail(ADC_EINVAL, "hip_stream is NULL");
    *hip_stream = (void *)e->stream;
    e->stream_exposed = true;           // (from now on the caller may enqueue on it without telling: launch_step)
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sample_actions(adc_engine *e, float bid_lo, float bid_hi, float budget)
{
    ENGINE_GUARD_STEP(e);
    return launch_chained(e, [&](const View &v, const PolicyView &, hipStream_t st, float *d_bids, float *d_budget) {
        hipLaunchKernelGGL(k_sample_actions, dim3((unsigned)((v.K + 255) / 256), (unsigned)v.N), dim3(256), 0, st, v, bid_lo, bid_hi, budget, d_bids, d_budget);
    });
}

ADC_EXPORT int adc_engine_set_flat_actions_device(adc_engine *e, const float *d_flat)
{
    ENGINE_GUARD(e);
    if (!d_flat) return fail(ADC_EINVAL, "flat action pointer is NULL");
    hipLaunchKernelGGL(k_unflatten_actions, dim3((unsigned)((e->v.K + 255) / 256), (unsigned)e->v.N), dim3(256), 0, e->stream, e->v,
                       d_flat, e->d_bids, e->d_budget);
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}

ADC_EXPORT int adc_engine_flat_obs_enable(adc_engine *e, int enabled)
{
    ENGINE_GUARD(e);
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (enabled && !e->d_flat_obs) {
        int rc = dev_alloc(e, &e->d_flat_obs, (size_t)e->v.N * (5 * (size_t)e->v.K + 2));
        if (rc) return rc;
    }
    e->v.flat_obs = enabled ? e->d_flat_obs : nullptr;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_profile_enable(adc_engine *e, int enabled)
{
    ENGINE_GUARD(e);
    if (enabled && e->ev.empty()) {
        e->ev.resize((size_t)kProfileRing * kProfileMarks);
        for (auto &ev : e->ev) HIP_TRY(hipEventCreate(&ev));
    }
    e->profiling = enabled != 0;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_profile_sample_every(adc_engine *e, int32_t every)
{
    ENGINE_GUARD(e);
    if (every < 1) return fail(ADC_EINVAL, "profile sampling interval must be >= 1");
    e->profile_every = every;
    e->profile_tick = 0;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_profile_read(adc_engine *e, double *kernel_ms_total, int64_t *launches)
{
    ENGINE_GUARD(e);
    int rc = flush_profile(e);
    if (rc) return rc;
    if (kernel_ms_total) for (int j = 0; j < 3; ++j) kernel_ms_total[j] = e->prof_ms[j];
    if (launches) *launches = e->prof_launches;
    e->prof_ms[0] = e->prof_ms[1] = e->prof_ms[2] = 0.0;
    e->prof_launches = 0;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_profile_records(adc_engine *e, int64_t *event_records)
{
    ENGINE_GUARD(e);
    if (!event_records) return fail(ADC_EINVAL, "event_records is NULL");
    *event_records = e->event_records;
    return ADC_OK;
}

// GPU time of a whole region of the engine's stream with ONE event pair (nothing per step): begin records an event, end records
// another, waits for it and returns the milliseconds in between - what a caller timing K steps on the host clock can check its
// figure against (the difference is launch latency and host overhead, not kernel time)
ADC_EXPORT int adc_engine_region_begin(adc_engine *e)
{
    ENGINE_GUARD(e);
    if (!e->region_ev[0]) for (hipEvent_t &ev : e->region_ev) HIP_TRY(hipEventCreate(&ev));
    HIP_TRY(hipEventRecord(e->region_ev[0], e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_region_end(adc_engine *e, double *gpu_ms)
{
    ENGINE_GUARD(e);
    if (!gpu_ms) return fail(ADC_EINVAL, "gpu_ms is NULL");
    if (!e->region_ev[0]) return fail(ADC_ESTATE, "adc_engine_region_begin has not been called");
    HIP_TRY(hipEventRecord(e->region_ev[1], e->stream));
    HIP_TRY(hipEventSynchronize(e->region_ev[1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->region_ev[0], e->region_ev[1]));
    *gpu_ms = ms;
    return ADC_OK;
}

ADC_EXPORT const char *adc_engine_step_kernel_name(adc_engine *e)
{
    if (!e) return "";
    return e->step_kernel;
}

ADC_EXPORT int adc_engine_metrics_enable(adc_engine *e, int enabled)
{
    ENGINE_GUARD(e);
    e->v.metrics_on = enabled ? 1 : 0;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_metrics_reset(adc_engine *e)
{
    ENGINE_GUARD(e);
    HIP_TRY(hipMemsetAsync(e->v.metric_profit, 0, (size_t)e->v.K * 8, e->stream));
    HIP_TRY(hipMemsetAsync(e->v.metric_scalars, 0, 64, e->stream));
    HIP_TRY(hipMemsetAsync(e->v.metric_env, 0, (size_t)e->v.N * 32, e->stream));
    HIP_TRY(hipMemsetAsync(e->v.metric_lo, 0, (size_t)e->v.N * e->v.K * 4, e->stream));
    HIP_TRY(hipMemsetAsync(e->v.metric_hi, 0, (size_t)e->v.N * e->v.K * 8, e->stream));
    if (e->have_ideal) {
        HIP_TRY(hipMemsetAsync(e->pol.sum_ideal, 0, (size_t)e->v.N * e->v.K * 8, e->stream));
        HIP_TRY(hipMemsetAsync(e->pol.sum_ideal_pos, 0, (size_t)e->v.N * e->v.K * 8, e->stream));
    }
    return ADC_OK;
}

ADC_EXPORT int adc_engine_metrics_read(adc_engine *e, int64_t *keyword_profit_cents_k, int64_t *scalars8)
{
    ENGINE_GUARD(e);
    if (keyword_profit_cents_k) {
        HIP_TRY(hipMemsetAsync(e->v.metric_profit, 0, (size_t)e->v.K * 8, e->stream));
        hipLaunchKernelGGL(k_metric_columns, dim3((unsigned)((e->v.K + 255) / 256), kColumnSlabs), dim3(256), 0, e->stream, e->v);
        HIP_TRY(hipGetLastError());
    }
    if (keyword_profit_cents_k) HIP_TRY(hipMemcpyAsync(keyword_profit_cents_k, e->v.metric_profit, (size_t)e->v.K * 8, hipMemcpyDeviceToHost, e->stream));
    if (scalars8) {
        hipLaunchKernelGGL(k_metric_reduce, dim3(4), dim3(256), 0, e->stream, e->v);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(scalars8, e->v.metric_scalars, 64, hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

namespace {
// the bid curves exist for the two single-competitor models; the reference's estimator on the default ImplicitKeyword's bidder pool
// sorts s x n bids and divides by n (an impression rate above 1), and no notebook uses it that way
int curves_model_check(const adc_engine *e, const char *what)
{
    if (e->v.model == ADC_MODEL_IMPLICIT || e->v.model == ADC_MODEL_EXPLICIT) return ADC_OK;
    return fail(ADC_EINVAL, std::string(what) + " is defined for IMPLICIT and EXPLICIT keywords (IMPLICIT_GENERAL: the reference's estimator "
                                                "on a bidder pool gives impression rates above 1)");
}
// EXPLICIT: the grid and its cost law, [3][n_bids] = bid, mu_b, sigma_b (adc::explicit_cost_law, float64 on the host)
std::vector<double> explicit_grid3(const double *bid_grid, int n_bids)
{
    std::vector<double> g(3 * (size_t)n_bids);
    for (int i = 0; i < n_bids; ++i) {
        g[i] = bid_grid[i];
        adc::explicit_cost_law(bid_grid[i], g[n_bids + i], g[2 * (size_t)n_bids + i]);
    }
    return g;
}
void launch_explicit_curves(const adc_engine *e, int n_samples, const double *d_grid3, int n_bids, double *ideal_out, float4 *curve_out)
{
    const size_t nk = (size_t)e->v.N * e->v.K;
    const dim3 grid(ideal_grid((long long)nk, e->num_cus, kIdealWaves)), block(kWave * kIdealWaves);
    if (n_samples <= kCachedSamples)
        hipLaunchKernelGGL(k_explicit_curves<true>, grid, block, 0, e->stream, e->v, n_samples, n_bids, d_grid3, d_grid3 + n_bids,
                           d_grid3 + 2 * (size_t)n_bids, ideal_out, curve_out, (long long)nk);
    else
        hipLaunchKernelGGL(k_explicit_curves<false>, grid, block, 0, e->stream, e->v, n_samples, n_bids, d_grid3, d_grid3 + n_bids,
                           d_grid3 + 2 * (size_t)n_bids, ideal_out, curve_out, (long long)nk);
}
// the per-step ideal on the cached curves: contender lists or (ADCRAFT_IDEAL_FULL_SCAN) the whole grid, for the engine's model
void launch_ideal_step(const View &v, const PolicyView &p, hipStream_t st, bool full_scan)
{
    const size_t nk = (size_t)v.N * v.K;
    if (v.model == ADC_MODEL_EXPLICIT) {
        if (full_scan) hipLaunchKernelGGL(k_ideal_from_curves<ADC_MODEL_EXPLICIT>, dim3((unsigned)((nk + 3) / 4)), dim3(256), 0, st, v, p, v.metrics_on);
        else hipLaunchKernelGGL(k_ideal_from_contenders<ADC_MODEL_EXPLICIT>, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, v, p, v.metrics_on);
    } else {
        if (full_scan) hipLaunchKernelGGL(k_ideal_from_curves<ADC_MODEL_IMPLICIT>, dim3((unsigned)((nk + 3) / 4)), dim3(256), 0, st, v, p, v.metrics_on);
        else hipLaunchKernelGGL(k_ideal_from_contenders<ADC_MODEL_IMPLICIT>, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, v, p, v.metrics_on);
    }
}
// the IMPLICIT estimator's limits (k_ideal_profit): 0, or ADC_EINVAL naming the one passed; *lim = the bins the grid keeps
int implicit_curve_args(int n_samples, const double *bid_grid, int n_bids, int *lim)
{
    if (n_samples > kIdealMaxSamples) return fail(ADC_EINVAL, "n_samples > 2^20 is not supported for IMPLICIT keywords (the estimator's 32-bit sums)");
    *lim = ideal_bins_kept(bid_grid, n_bids);
    if (*lim == 0) return fail(ADC_EINVAL, "bid grid: every bid must be finite and at most $20.46 (2046 cents) for IMPLICIT keywords");
    return 0;
}
void launch_ideal_profit(const View &v, hipStream_t st, int num_cus, int n_samples, int n_bids, const double *d_grid, const int32_t *tape,
                         double *ideal, double *ir, double *cpc, uint2 *packed, int lim, long long n_items)
{
    const int waves = ideal_waves(lim);
    hipLaunchKernelGGL(k_ideal_profit, dim3(ideal_grid(n_items, num_cus, waves)), dim3(kWave * waves), ideal_lds_bytes(lim, waves), st, v, n_samples,
                       n_bids, d_grid, tape, ideal, ir, cpc, packed, lim, n_items);
}
}  // namespace

ADC_EXPORT int adc_engine_ideal_profit(adc_engine *e, int n_samples, const double *bid_grid, int n_bids, double *host_nk)
{
    ENGINE_GUARD(e);
    if (int rc = curves_model_check(e, "ideal profit")) return rc;
    if (n_samples <= 0 || !host_nk || !bid_grid || n_bids <= 0) return fail(ADC_EINVAL, "bad arguments");
    const size_t nk = (size_t)e->v.N * e->v.K;
    if (e->v.model == ADC_MODEL_EXPLICIT) {
        if (n_samples > (1 << 20)) return fail(ADC_EINVAL, "n_samples > 2^20 is not supported for EXPLICIT keywords");
        if (e->v.drift_on) { materialize_drift(e); HIP_TRY(hipGetLastError()); }
        const std::vector<double> g3 = explicit_grid3(bid_grid, n_bids);
        double *d_out = nullptr, *d_grid = nullptr;
        HIP_TRY(hipMalloc((void **)&d_out, nk * 8));
        hipError_t err = hipMalloc((void **)&d_grid, g3.size() * 8);
        if (err == hipSuccess) err = hipMemcpyAsync(d_grid, g3.data(), g3.size() * 8, hipMemcpyHostToDevice, e->stream);
        if (err == hipSuccess) {
            launch_explicit_curves(e, n_samples, d_grid, n_bids, d_out, (float4 *)nullptr);
            err = hipGetLastError();
        }
        if (err == hipSuccess) err = hipMemcpyAsync(host_nk, d_out, nk * 8, hipMemcpyDeviceToHost, e->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
        (void)hipFree(d_out);
        (void)hipFree(d_grid);
        HIP_TRY(err);
        return ADC_OK;
    }
    int lim = 0;
    if (int rc = implicit_curve_args(n_samples, bid_grid, n_bids, &lim)) return rc;
    if (e->v.drift_on) { materialize_drift(e); HIP_TRY(hipGetLastError()); }
    double *d_out = nullptr, *d_grid = nullptr;
    HIP_TRY(hipMalloc((void **)&d_out, nk * 8));
    hipError_t err = hipMalloc((void **)&d_grid, (size_t)n_bids * 8);
    if (err == hipSuccess) err = hipMemcpyAsync(d_grid, bid_grid, (size_t)n_bids * 8, hipMemcpyHostToDevice, e->stream);
    if (err == hipSuccess) {
        launch_ideal_profit(e->v, e->stream, e->num_cus, n_samples, n_bids, d_grid, (const int32_t *)nullptr, d_out, (double *)nullptr, (double *)nullptr,
                            (uint2 *)nullptr, lim, (long long)nk);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipMemcpyAsync(host_nk, d_out, nk * 8, hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    (void)hipFree(d_out);
    (void)hipFree(d_grid);
    HIP_TRY(err);
    return ADC_OK;
}

// the estimator alone, on caller-supplied samples (cents, >= 0) of ONE keyword and any bid grid the estimator takes (pins the kernel
// against the reference's get_implicit_kw_bid_cpc_impressions).  Arguments are checked before any HIP call
ADC_EXPORT int adc_bid_curves_from_samples(int device_id, const int32_t *samples_cents, int32_t n_samples, const double *bid_grid,
                                           int32_t n_bids, double *impression_rate_out, double *cpc_out)
{
    if (!samples_cents || n_samples <= 0 || n_bids <= 0 || !bid_grid || !impression_rate_out || !cpc_out)
        return fail(ADC_EINVAL, "bad arguments");
    int lim = 0;
    if (int rc = implicit_curve_args(n_samples, bid_grid, n_bids, &lim)) return rc;
    for (int32_t i = 0; i < n_samples; ++i)
        if (samples_cents[i] < 0) return fail(ADC_EINVAL, "a negative sample (cents)");
    HIP_TRY(hipSetDevice(device_id));
    int32_t *d_s = nullptr;
    double *d_ir = nullptr, *d_cpc = nullptr, *d_grid = nullptr;
    float *d_p = nullptr;
    uint64_t *d_key = nullptr;
    uint32_t *d_tick = nullptr;
    auto done = [&](int code) { (void)hipFree(d_s); (void)hipFree(d_ir); (void)hipFree(d_cpc); (void)hipFree(d_p); (void)hipFree(d_key); (void)hipFree(d_tick); (void)hipFree(d_grid); return code; };
    if (hipMalloc((void **)&d_s, (size_t)n_samples * 4) != hipSuccess || hipMalloc((void **)&d_ir, (size_t)n_bids * 8) != hipSuccess ||
        hipMalloc((void **)&d_cpc, (size_t)n_bids * 8) != hipSuccess || hipMalloc((void **)&d_p, ADC_P_COUNT * 4) != hipSuccess ||
        hipMalloc((void **)&d_key, 8) != hipSuccess || hipMalloc((void **)&d_tick, 4) != hipSuccess ||
        hipMalloc((void **)&d_grid, (size_t)n_bids * 8) != hipSuccess)
        return done(fail(ADC_ENOMEM, "hipMalloc failed"));
    if (hipMemcpy(d_grid, bid_grid, (size_t)n_bids * 8, hipMemcpyHostToDevice) != hipSuccess) return done(fail(ADC_EHIP, "upload failed"));
    if (hipMemcpy(d_s, samples_cents, (size_t)n_samples * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemset(d_p, 0, ADC_P_COUNT * 4) != hipSuccess ||
        hipMemset(d_key, 0, 8) != hipSuccess || hipMemset(d_tick, 0, 4) != hipSuccess)
        return done(fail(ADC_EHIP, "upload failed"));
    View v;
    std::memset(&v, 0, sizeof(v));
    v.N = 1; v.K = 1; v.params = d_p; v.key = d_key; v.tick = d_tick;
    v.NP = 1;
    launch_ideal_profit(v, 0, 1, n_samples, n_bids, d_grid, d_s, (double *)nullptr, d_ir, d_cpc, (uint2 *)nullptr, lim, 1LL);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return done(fail(ADC_EHIP, "k_ideal_profit failed"));
    if (hipMemcpy(impression_rate_out, d_ir, (size_t)n_bids * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(cpc_out, d_cpc, (size_t)n_bids * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return done(fail(ADC_EHIP, "download failed"));
    return done(ADC_OK);
}

// adc_law.h win_brackets evaluated by the device (k_debug_win_brackets), 8 words per keyword: tests check them against the
// exact intervals on the host (adc_check_win_brackets)
ADC_EXPORT int adc_debug_win_brackets_device(int device_id, int64_t n, const float *bid, const float *cost_loc, const float *cost_scale,
                                             const float *buyside_ctr, uint32_t *out8)
{
    if (n < 0 || n > (1 << 26)) return fail(ADC_EINVAL, "n out of range");
    if (n == 0) return ADC_OK;
    if (!bid || !cost_loc || !cost_scale || !buyside_ctr || !out8) return fail(ADC_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(device_id));
    float *d_in = nullptr;
    uint32_t *d_out = nullptr;
    auto done = [&](int code) {
        if (d_in) (void)hipFree(d_in);
        if (d_out) (void)hipFree(d_out);
        return code;
    };
    const size_t m = (size_t)n;
    if (hipMalloc((void **)&d_in, 4 * m * 4) != hipSuccess || hipMalloc((void **)&d_out, 8 * m * 4) != hipSuccess) return done(fail(ADC_ENOMEM, "hipMalloc failed"));
    const float *src[4] = {bid, cost_loc, cost_scale, buyside_ctr};
    for (int i = 0; i < 4; ++i)
        if (hipMemcpy(d_in + i * m, src[i], m * 4, hipMemcpyHostToDevice) != hipSuccess) return done(fail(ADC_EHIP, "upload failed"));
    hipLaunchKernelGGL(k_debug_win_brackets, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, (int)n, d_in, d_in + m, d_in + 2 * m, d_in + 3 * m, d_out);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return done(fail(ADC_EHIP, "k_debug_win_brackets failed"));
    if (hipMemcpy(out8, d_out, 8 * m * 4, hipMemcpyDeviceToHost) != hipSuccess) return done(fail(ADC_EHIP, "download failed"));
    return done(ADC_OK);
}

// Philox4x32 (the stream's round count) evaluated by the device for n (counter, key) pairs - the GPU side of the stream battery
ADC_EXPORT int adc_debug_walk_stats(adc_engine *e, int64_t stats[4], int reset)
{
    ENGINE_GUARD(e);
    if (!stats) return fail(ADC_EINVAL, "stats is NULL");
    HIP_TRY(hipStreamSynchronize(e->stream));
    unsigned long long h[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_walk_stats), sizeof(h)));
    for (int i = 0; i < 4; ++i) stats[i] = (int64_t)h[i];
#ifdef ADC_EXP_TIMING
    {   // timing build: the phase sums go to stderr (setup | sort | walk | commit | gather | second part | groups | candidates)
        unsigned long long ph[20];
        HIP_TRY(hipMemcpyFromSymbol(ph, HIP_SYMBOL(g_walk_phase), 8 * sizeof(ph[0])));
        std::fprintf(stderr, "walk phases:");
        for (int i = 0; i < 8; ++i) std::fprintf(stderr, " %llu", ph[i]);
        std::fprintf(stderr, "\n");
        HIP_TRY(hipMemcpyFromSymbol(ph, HIP_SYMBOL(g_rest_phase), sizeof(ph)));
        std::fprintf(stderr, "rest-of-day phases (10 ns ticks: pass over the auctions | of which laws | marked cells | outputs | envs | cells walked | of which paid / marks | - | "
                             "list of the marks | k_rest_walk: before the walk | chunks resolved | whole env | slowest env | chunk: cells | chain | paid | at-once variant: own cells | chain | commit | envs):");
        for (int i = 0; i < 20; ++i) std::fprintf(stderr, " %llu", ph[i]);
        std::fprintf(stderr, "\n");
        if (reset) {
            const unsigned long long z8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_walk_phase), z8, sizeof(z8)));
            const unsigned long long z16[20] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_rest_phase), z16, sizeof(z16)));
        }
    }
#endif
    if (reset) {
        const unsigned long long z[4] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_walk_stats), z, sizeof(z)));
    }
    return ADC_OK;
}

ADC_EXPORT int adc_debug_direct_days(adc_engine *e, int64_t *env_days, int reset)
{
    ENGINE_GUARD(e);
    if (!env_days) return fail(ADC_EINVAL, "env_days is NULL");
    HIP_TRY(hipStreamSynchronize(e->stream));
    unsigned long long h = 0;
    if (e->v.direct_days) {             // (null: this engine never parks an env at once - K > 256, fewer than 1024 envs, another model)
        HIP_TRY(hipMemcpy(&h, e->v.direct_days, sizeof(h), hipMemcpyDeviceToHost));
        if (reset) HIP_TRY(hipMemset(e->v.direct_days, 0, sizeof(h)));
    }
    *env_days = (int64_t)h;
    return ADC_OK;
}

ADC_EXPORT int adc_debug_philox_device(int device_id, int64_t n, const uint32_t *ctr4, const uint32_t *key2, uint32_t *out4)
{
    if (n < 0 || n > (1 << 26)) return fail(ADC_EINVAL, "n out of range");
    if (n == 0) return ADC_OK;
    if (!ctr4 || !key2 || !out4) return fail(ADC_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(device_id));
    uint32_t *d = nullptr;
    const size_t m = (size_t)n;
    if (hipMalloc((void **)&d, 10 * m * 4) != hipSuccess) return fail(ADC_ENOMEM, "hipMalloc failed");
    auto done = [&](int code) { (void)hipFree(d); return code; };
    if (hipMemcpy(d, ctr4, 4 * m * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d + 4 * m, key2, 2 * m * 4, hipMemcpyHostToDevice) != hipSuccess)
        return done(fail(ADC_EHIP, "upload failed"));
    hipLaunchKernelGGL(k_debug_philox, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, (int)n, d, d + 4 * m, d + 6 * m);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return done(fail(ADC_EHIP, "k_debug_philox failed"));
    if (hipMemcpy(out4, d + 6 * m, 4 * m * 4, hipMemcpyDeviceToHost) != hipSuccess) return done(fail(ADC_EHIP, "download failed"));
    return done(ADC_OK);
}

ADC_EXPORT int adc_debug_chain_device(int device_id, double r0, int64_t n, const double *x, double *out2)
{
    if (n < 0 || n > (1 << 24)) return fail(ADC_EINVAL, "n out of range");
    if ((n > 0 && !x) || !out2) return fail(ADC_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(device_id));
    double *d = nullptr;
    if (hipMalloc((void **)&d, ((size_t)n + 2) * 8) != hipSuccess) return fail(ADC_ENOMEM, "hipMalloc failed");
    auto done = [&](int code) { (void)hipFree(d); return code; };
    if (n > 0 && hipMemcpy(d + 2, x, (size_t)n * 8, hipMemcpyHostToDevice) != hipSuccess) return done(fail(ADC_EHIP, "upload failed"));
    hipLaunchKernelGGL(k_debug_chain, dim3(1), dim3(kWave), 0, 0, r0, (int)n, d + 2, d);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return done(fail(ADC_EHIP, "k_debug_chain failed"));
    if (hipMemcpy(out2, d, 16, hipMemcpyDeviceToHost) != hipSuccess) return done(fail(ADC_EHIP, "download failed"));
    return done(ADC_OK);
}

ADC_EXPORT int adc_nth_price_auction(int device_id, double bid, const double *other_bids, int32_t n_auctions, int32_t n_bidders,
                                     int32_t n, int32_t num_winners, int32_t *impressions, int32_t *placements, double *costs)
{
    if (!impressions) return fail(ADC_EINVAL, "impressions is NULL");
    *impressions = 0;
    if (n < 1 || num_winners < 1 || n + num_winners > kTopMax) return fail(ADC_EINVAL, "need n >= 1, num_winners >= 1, n + num_winners <= 32");
    if (n_auctions < 0 || n_bidders < 0) return fail(ADC_EINVAL, "negative shape");
    if (n_auctions == 0) return ADC_OK;
    if (n_bidders > 0 && !other_bids) return fail(ADC_EINVAL, "other_bids is NULL");
    HIP_TRY(hipSetDevice(device_id));
    double *d_other = nullptr, *d_cost = nullptr;
    int *d_won = nullptr, *d_place = nullptr;
    const size_t na = n_auctions, nb = n_bidders;
    int rc = ADC_OK;
    auto done = [&](int code) {
        if (d_other) (void)hipFree(d_other);
        if (d_cost) (void)hipFree(d_cost);
        if (d_won) (void)hipFree(d_won);
        if (d_place) (void)hipFree(d_place);
        return code;
    };
    if (hipMalloc((void **)&d_other, (na * nb ? na * nb : 1) * 8) != hipSuccess || hipMalloc((void **)&d_cost, na * 8) != hipSuccess ||
        hipMalloc((void **)&d_won, na * 4) != hipSuccess || hipMalloc((void **)&d_place, na * 4) != hipSuccess)
        return done(fail(ADC_ENOMEM, "hipMalloc failed"));
    if (na * nb && hipMemcpy(d_other, other_bids, na * nb * 8, hipMemcpyHostToDevice) != hipSuccess) return done(fail(ADC_EHIP, "upload failed"));
    hipLaunchKernelGGL(k_nth_price, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, 0, bid, d_other, n_auctions, n_bidders, n, num_winners, d_won, d_place, d_cost);
    if (hipGetLastError() != hipSuccess) return done(fail(ADC_EHIP, "k_nth_price launch failed"));
    std::vector<int> won(na), place(na);
    std::vector<double> cost(na);
    if (hipMemcpy(won.data(), d_won, na * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(place.data(), d_place, na * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(cost.data(), d_cost, na * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return done(fail(ADC_EHIP, "download failed"));
    int32_t m = 0;
    for (size_t a = 0; a < na; ++a)
        if (won[a]) {
            if (placements) placements[m] = place[a];
            if (costs) costs[m] = cost[a];
            ++m;
        }
    *impressions = m;
    return done(rc);
}


// ---- baseline policies and the per-step ideal, device-resident (kernels_policy.inc) -----------------------------------
namespace {
int ensure_ideal_buffers(adc_engine *e)
{
    if (e->have_ideal) return ADC_OK;
    const size_t nk = (size_t)e->v.N * e->v.K;
    int rc;
    if ((rc = dev_alloc(e, &e->pol.ideal, nk))) return rc;
    if ((rc = dev_alloc(e, &e->pol.best, nk))) return rc;
    if ((rc = dev_alloc(e, &e->pol.sum_ideal, nk))) return rc;
    if ((rc = dev_alloc(e, &e->pol.sum_ideal_pos, nk))) return rc;
    e->have_ideal = true;
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_agent_init(adc_engine *e, float default_rpc, const uint64_t *seeds_n)
{
    ENGINE_GUARD(e);
    const size_t N = e->v.N, nk = N * e->v.K;
    if (!e->have_agent) {
        int rc;
        if ((rc = dev_alloc(e, &e->pol.ave_rpc, nk))) return rc;
        if ((rc = dev_alloc(e, &e->pol.n_rpc, nk))) return rc;
        if ((rc = dev_alloc(e, &e->pol.ave_sctr, nk))) return rc;
        if ((rc = dev_alloc(e, &e->pol.n_sctr, nk))) return rc;
        if ((rc = dev_alloc(e, &e->pol.max_bid, nk))) return rc;
        if ((rc = dev_alloc(e, &e->pol.key, N))) return rc;
        if ((rc = dev_alloc(e, &e->pol.tick, N))) return rc;
        e->have_agent = true;
    }
    e->pol.default_rpc = default_rpc;
    uint64_t *d_seeds = nullptr;
    if (seeds_n) { HIP_TRY(hipMalloc((void **)&d_seeds, N * 8)); HIP_TRY(hipMemcpyAsync(d_seeds, seeds_n, N * 8, hipMemcpyHostToDevice, e->stream)); }
    hipLaunchKernelGGL(k_agent_init, dim3((unsigned)((e->v.K + 255) / 256), (unsigned)N), dim3(256), 0, e->stream, e->v, e->pol, d_seeds,
                       e->cfg.seed, e->cfg.env_id_base);
    hipError_t err = hipGetLastError();
    hipError_t err2 = hipStreamSynchronize(e->stream);
    if (d_seeds) (void)hipFree(d_seeds);
    HIP_TRY(err);
    HIP_TRY(err2);
    return ADC_OK;
}

namespace {
// update and/or act; host observation arrays (all three or none) are staged through temporaries
int agent_launch(adc_engine *e, const int32_t *clicks_nk, const int32_t *conv_nk, const float *rev_nk, int do_update, int do_act,
                 const double *replay_u_nk, float budget_override)
{
    if (!e->have_agent) return fail(ADC_ESTATE, "adc_engine_agent_init has not been called");
    const int given = (clicks_nk != nullptr) + (conv_nk != nullptr) + (rev_nk != nullptr);
    if (given != 0 && given != 3) return fail(ADC_EINVAL, "pass all of clicks/conversions/revenue, or none (= the engine's last observation)");
    const size_t nk = (size_t)e->v.N * e->v.K;
    int32_t *d_clk = nullptr, *d_conv = nullptr;
    float *d_rev = nullptr;
    double *d_u = nullptr;
    auto done = [&](hipError_t err) {
        hipError_t e2 = (d_clk || d_u) ? hipStreamSynchronize(e->stream) : hipSuccess;
        (void)hipFree(d_clk); (void)hipFree(d_conv); (void)hipFree(d_rev); (void)hipFree(d_u);
        if (err != hipSuccess) return fail(ADC_EHIP, hipGetErrorString(err));
        if (e2 != hipSuccess) return fail(ADC_EHIP, hipGetErrorString(e2));
        return (int)ADC_OK;
    };
    hipError_t err = hipSuccess;
    if (given == 3 && do_update) {
        if (hipMalloc((void **)&d_clk, nk * 4) != hipSuccess || hipMalloc((void **)&d_conv, nk * 4) != hipSuccess ||
            hipMalloc((void **)&d_rev, nk * 4) != hipSuccess) { (void)done(hipSuccess); return fail(ADC_ENOMEM, "hipMalloc failed"); }
        err = hipMemcpyAsync(d_clk, clicks_nk, nk * 4, hipMemcpyHostToDevice, e->stream);
        if (err == hipSuccess) err = hipMemcpyAsync(d_conv, conv_nk, nk * 4, hipMemcpyHostToDevice, e->stream);
        if (err == hipSuccess) err = hipMemcpyAsync(d_rev, rev_nk, nk * 4, hipMemcpyHostToDevice, e->stream);
    }
    if (err == hipSuccess && replay_u_nk && do_act) {
        if (hipMalloc((void **)&d_u, nk * 8) != hipSuccess) { (void)done(hipSuccess); return fail(ADC_ENOMEM, "hipMalloc failed"); }
        err = hipMemcpyAsync(d_u, replay_u_nk, nk * 8, hipMemcpyHostToDevice, e->stream);
    }
    if (err == hipSuccess) {
        hipLaunchKernelGGL(k_agent_step, dim3((unsigned)e->v.N), dim3(256), 0, e->stream, e->v, e->pol,
                           d_clk ? d_clk : e->v.clk, d_conv ? d_conv : e->v.conv, d_rev ? d_rev : e->v.rev, do_update, do_act,
                           (const double *)d_u, budget_override, e->d_bids, e->d_budget);
        err = hipGetLastError();
    }
    return done(err);
}
}  // namespace

namespace {
// update + act on the engine's last observation (no host arrays): chain-compatible
int agent_step_chained(adc_engine *e, float budget_override)
{
    if (!e->have_agent) return fail(ADC_ESTATE, "adc_engine_agent_init has not been called");
    return launch_chained(e, [&](const View &v, const PolicyView &p, hipStream_t st, float *d_bids, float *d_budget) {
        hipLaunchKernelGGL(k_agent_step, dim3((unsigned)v.N), dim3(256), 0, st, v, p, v.clk, v.conv, v.rev, 1, 1, (const double *)nullptr, budget_override, d_bids, d_budget);
    });
}
}  // namespace

ADC_EXPORT int adc_engine_agent_update(adc_engine *e, const int32_t *clicks_nk, const int32_t *conversions_nk, const float *revenue_nk)
{
    ENGINE_GUARD(e);
    return agent_launch(e, clicks_nk, conversions_nk, revenue_nk, 1, 0, nullptr, 0.0f);
}

ADC_EXPORT int adc_engine_agent_act(adc_engine *e, float budget_override, const double *replay_uniforms_nk)
{
    ENGINE_GUARD(e);
    return agent_launch(e, nullptr, nullptr, nullptr, 0, 1, replay_uniforms_nk, budget_override);
}

ADC_EXPORT int adc_engine_agent_step(adc_engine *e, float budget_override)
{
    ENGINE_GUARD_STEP(e);
    return agent_step_chained(e, budget_override);
}

ADC_EXPORT int adc_engine_agent_state(adc_engine *e, float *ave_rpc_nk, int32_t *num_rpc_obs_nk, float *ave_sctr_nk,
                                      int32_t *num_sctr_obs_nk, double *max_bids_nk)
{
    ENGINE_GUARD(e);
    if (!e->have_agent) return fail(ADC_ESTATE, "adc_engine_agent_init has not been called");
    const size_t nk = (size_t)e->v.N * e->v.K;
    if (ave_rpc_nk) HIP_TRY(hipMemcpyAsync(ave_rpc_nk, e->pol.ave_rpc, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (num_rpc_obs_nk) HIP_TRY(hipMemcpyAsync(num_rpc_obs_nk, e->pol.n_rpc, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (ave_sctr_nk) HIP_TRY(hipMemcpyAsync(ave_sctr_nk, e->pol.ave_sctr, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (num_sctr_obs_nk) HIP_TRY(hipMemcpyAsync(num_sctr_obs_nk, e->pol.n_sctr, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (max_bids_nk) HIP_TRY(hipMemcpyAsync(max_bids_nk, e->pol.max_bid, nk * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_get_actions(adc_engine *e, float *bids_nk, float *budget_n)
{
    ENGINE_GUARD(e);
    if (bids_nk) HIP_TRY(hipMemcpyAsync(bids_nk, e->d_bids, (size_t)e->v.N * e->v.K * 4, hipMemcpyDeviceToHost, e->stream));
    if (budget_n) HIP_TRY(hipMemcpyAsync(budget_n, e->d_budget, (size_t)e->v.N * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_bid_curves_build(adc_engine *e, int n_samples, const double *bid_grid, int n_bids)
{
    ENGINE_GUARD(e);
    if (int rc = curves_model_check(e, "bid curves")) return rc;
    if (n_samples <= 0 || !bid_grid || n_bids <= 0) return fail(ADC_EINVAL, "bad arguments");
    const bool xp = e->v.model == ADC_MODEL_EXPLICIT;
    int lim = 0;
    if (!xp) if (int rc = implicit_curve_args(n_samples, bid_grid, n_bids, &lim)) return rc;      // (before the cached curves are touched)
    const size_t nk = (size_t)e->v.N * e->v.K;
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (n_samples > (1 << 20)) return fail(ADC_EINVAL, "n_samples > 2^20 is not supported for cached curves");
    if (!e->have_curves || e->pol.n_bids != n_bids) {
        for (void *p : e->curve_allocs) (void)hipFree(p);
        e->curve_allocs.clear();
        e->have_curves = false;
        void *curve = nullptr, *grid = nullptr, *cont = nullptr, *ncont = nullptr, *cpos = nullptr;
        // contender lists: 24 bytes per distinct grid point that can be the argmax (typically half of the grid); curves with more
        // points than a list holds are evaluated on the whole grid
        const int cap = std::min(n_bids, 256);
        // (EXPLICIT: 16 bytes per keyword instead of 8 per grid point, and the grid's cost law beside the grid)
        const size_t curve_bytes = xp ? nk * sizeof(float4) : nk * n_bids * sizeof(uint2);
        if (hipMalloc(&curve, curve_bytes) != hipSuccess || hipMalloc(&grid, (size_t)n_bids * 8 * (xp ? 3 : 1)) != hipSuccess ||
            hipMalloc(&cont, nk * cap * sizeof(ContenderEntry)) != hipSuccess ||
            hipMalloc(&ncont, nk * sizeof(uint16_t)) != hipSuccess || hipMalloc(&cpos, nk * sizeof(uint16_t)) != hipSuccess) {
            (void)hipFree(curve); (void)hipFree(grid); (void)hipFree(cont); (void)hipFree(ncont); (void)hipFree(cpos);
            return fail(ADC_ENOMEM, "bid curves need ~30 bytes x num_envs x num_keywords x n_bids of device memory");
        }
        e->curve_allocs = {curve, grid, cont, ncont, cpos};
        if (xp) {
            e->pol.xcurve = (float4 *)curve;
            e->pol.grid_mu = (double *)grid + n_bids;
            e->pol.grid_sigma = (double *)grid + 2 * (size_t)n_bids;
        } else {
            e->pol.curve = (uint2 *)curve;
        }
        e->pol.grid = (double *)grid; e->pol.n_bids = n_bids;
        e->pol.contender = (ContenderEntry *)cont; e->pol.n_contenders = (uint16_t *)ncont;
        e->pol.cont_pos = (uint16_t *)cpos; e->pol.cont_cap = cap;
        e->have_curves = true;
    }
    e->pol.n_samples = n_samples;
    int rc = ensure_ideal_buffers(e);
    if (rc) return rc;
    if (xp) {
        const std::vector<double> g3 = explicit_grid3(bid_grid, n_bids);
        HIP_TRY(hipMemcpyAsync(e->pol.grid, g3.data(), g3.size() * 8, hipMemcpyHostToDevice, e->stream));
        launch_explicit_curves(e, n_samples, e->pol.grid, n_bids, (double *)nullptr, e->pol.xcurve);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(e->stream));       // (g3 is a host temporary)
    } else {
    HIP_TRY(hipMemcpyAsync(e->pol.grid, bid_grid, (size_t)n_bids * 8, hipMemcpyHostToDevice, e->stream));
    launch_ideal_profit(e->v, e->stream, e->num_cus, n_samples, n_bids, e->pol.grid, (const int32_t *)nullptr, (double *)nullptr, (double *)nullptr,
                        (double *)nullptr, e->pol.curve, lim, (long long)nk);
    HIP_TRY(hipGetLastError());
    }
    // which grid points can be the argmax at all (k_curve_contenders): the per-step ideal then evaluates only those
    HIP_TRY(hipMemsetAsync(e->pol.cont_pos, 0, nk * sizeof(uint16_t), e->stream));
    if (n_bids <= kContenderLines) {
        if (xp) hipLaunchKernelGGL(k_curve_contenders<ADC_MODEL_EXPLICIT>, dim3((unsigned)nk), dim3(kWave), sizeof(ContenderScratch), e->stream, e->v, e->pol);
        else hipLaunchKernelGGL(k_curve_contenders<ADC_MODEL_IMPLICIT>, dim3((unsigned)nk), dim3(kWave), sizeof(ContenderScratch), e->stream, e->v, e->pol);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemsetAsync(e->pol.n_contenders, 0xFF, nk * sizeof(uint16_t), e->stream));       // kContenderAll: the whole grid
    }
    HIP_TRY(hipStreamSynchronize(e->stream));      // (bid_grid is only borrowed)
    return ADC_OK;
}

ADC_EXPORT int adc_engine_bid_curves_fetch(adc_engine *e, double *impression_rate_host, double *cpc_host)
{
    ENGINE_GUARD(e);
    if (!e->have_curves) return fail(ADC_ESTATE, "adc_engine_bid_curves_build has not been called");
    const size_t n = (size_t)e->v.N * e->v.K * e->pol.n_bids;
    if (e->v.model == ADC_MODEL_EXPLICIT) {          // the points evaluated on the device, by the function every ideal kernel calls
        double *d = nullptr;
        if (hipMalloc((void **)&d, 2 * n * 8) != hipSuccess) return fail(ADC_ENOMEM, "hipMalloc failed");
        const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, (size_t)e->num_cus * 64));
        hipLaunchKernelGGL(k_explicit_curve_points, dim3(blocks), dim3(256), 0, e->stream, e->v, e->pol, d, d + n);
        hipError_t err = hipGetLastError();
        if (err == hipSuccess && impression_rate_host) err = hipMemcpyAsync(impression_rate_host, d, n * 8, hipMemcpyDeviceToHost, e->stream);
        if (err == hipSuccess && cpc_host) err = hipMemcpyAsync(cpc_host, d + n, n * 8, hipMemcpyDeviceToHost, e->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
        (void)hipFree(d);
        HIP_TRY(err);
        return ADC_OK;
    }
    std::vector<uint2> packed(n);
    HIP_TRY(hipMemcpyAsync(packed.data(), e->pol.curve, n * sizeof(uint2), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const double ns = (double)e->pol.n_samples;
    for (size_t i = 0; i < n; ++i) {            // the same IEEE operations k_ideal_from_curves applies
        const unsigned int idx = packed[i].y & 0x7FFFFFFFu;
        if (impression_rate_host) impression_rate_host[i] = (double)idx / ns;
        if (cpc_host) cpc_host[i] = ((double)packed[i].x / 100.0) / ((packed[i].y >> 31) ? ns : (double)(idx + 1u));
    }
    return ADC_OK;
}

// the contender lists of the cached curves (k_curve_contenders): n_nk[N*K] (0xFFFF = "the whole grid"), per entry 6 words
// {margin interval lo, hi (float32 bits), curve point x, y, grid index, 0}
ADC_EXPORT int adc_engine_bid_curves_contenders(adc_engine *e, uint16_t *n_nk, uint32_t *entries_nkc6, int32_t *cap)
{
    ENGINE_GUARD(e);
    if (!e->have_curves) return fail(ADC_ESTATE, "adc_engine_bid_curves_build has not been called");
    const size_t nk = (size_t)e->v.N * e->v.K;
    if (cap) *cap = e->pol.cont_cap;
    if (n_nk) HIP_TRY(hipMemcpyAsync(n_nk, e->pol.n_contenders, nk * 2, hipMemcpyDeviceToHost, e->stream));
    if (entries_nkc6) HIP_TRY(hipMemcpyAsync(entries_nkc6, e->pol.contender, nk * e->pol.cont_cap * sizeof(ContenderEntry), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

namespace {
// the per-step ideal of every keyword into the device-side arrays and running sums (nothing to the host): chain-compatible
int ideal_step_chained(adc_engine *e)
{
    if (!e->have_curves) return fail(ADC_ESTATE, "adc_engine_bid_curves_build has not been called");
    const bool full_scan = e->ideal_full_scan;
    const int rc = launch_chained(e, [&](const View &v, const PolicyView &p, hipStream_t st, float *, float *) {
        // the reference evaluates env.keyword_params as they stand before the step, i.e. with the last update_keywords applied
        if (v.drift_on) hipLaunchKernelGGL(k_materialize_drift, dim3(v.N), dim3(256), 0, st, v);
        launch_ideal_step(v, p, st, full_scan);
    });
    if (!rc && e->v.drift_on) e->drift_applied = true;
    return rc;
}
int policy_oracle_chained(adc_engine *e, float budget)
{
    if (!e->have_curves) return fail(ADC_ESTATE, "adc_engine_bid_curves_build / adc_engine_ideal_step have not been called");
    return launch_chained(e, [&](const View &v, const PolicyView &p, hipStream_t st, float *d_bids, float *d_budget) {
        hipLaunchKernelGGL(k_policy_oracle, dim3((unsigned)((v.K + 255) / 256), (unsigned)v.N), dim3(256), 0, st, v, p, budget, d_bids, d_budget);
    });
}
}  // namespace

ADC_EXPORT int adc_engine_ideal_step(adc_engine *e, double *ideal_host_nk, int32_t *best_index_host_nk)
{
    if (e && !ideal_host_nk && !best_index_host_nk) {
        ENGINE_GUARD_STEP(e);
        return ideal_step_chained(e);
    }
    ENGINE_GUARD(e);
    if (!e->have_curves) return fail(ADC_ESTATE, "adc_engine_bid_curves_build has not been called");
    const size_t nk = (size_t)e->v.N * e->v.K;
    // the reference evaluates env.keyword_params as they stand before the step, i.e. with the last update_keywords applied
    if (e->v.drift_on) { materialize_drift(e); HIP_TRY(hipGetLastError()); }
    launch_ideal_step(e->v, e->pol, e->stream, e->ideal_full_scan);
    HIP_TRY(hipGetLastError());
    if (ideal_host_nk) HIP_TRY(hipMemcpyAsync(ideal_host_nk, e->pol.ideal, nk * 8, hipMemcpyDeviceToHost, e->stream));
    if (best_index_host_nk) HIP_TRY(hipMemcpyAsync(best_index_host_nk, e->pol.best, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (ideal_host_nk || best_index_host_nk) HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_policy_oracle(adc_engine *e, float budget)
{
    ENGINE_GUARD_STEP(e);
    return policy_oracle_chained(e, budget);
}

ADC_EXPORT int adc_engine_metrics_read_nk(adc_engine *e, int64_t *profit_cents_nk, double *ideal_sum_nk, double *ideal_pos_sum_nk)
{
    ENGINE_GUARD(e);
    const size_t nk = (size_t)e->v.N * e->v.K;
    if ((ideal_sum_nk || ideal_pos_sum_nk) && !e->have_ideal) return fail(ADC_ESTATE, "no ideal profit has been accumulated (adc_engine_ideal_step)");
    std::vector<int32_t> lo;
    if (profit_cents_nk) {          // the 64-bit spill into the caller's array, the 32-bit words beside it: added below
        lo.resize(nk);
        HIP_TRY(hipMemcpyAsync(profit_cents_nk, e->v.metric_hi, nk * 8, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipMemcpyAsync(lo.data(), e->v.metric_lo, nk * 4, hipMemcpyDeviceToHost, e->stream));
    }
    if (ideal_sum_nk) HIP_TRY(hipMemcpyAsync(ideal_sum_nk, e->pol.sum_ideal, nk * 8, hipMemcpyDeviceToHost, e->stream));
    if (ideal_pos_sum_nk) HIP_TRY(hipMemcpyAsync(ideal_pos_sum_nk, e->pol.sum_ideal_pos, nk * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < lo.size(); ++i) profit_cents_nk[i] += lo[i];
    return ADC_OK;
}

// per-env AKNCP and NCP of the running episode, reduced on the device (k_akncp_ncp)
ADC_EXPORT int adc_engine_metrics_akncp_ncp(adc_engine *e, double days, double *akncp_n, double *ncp_n)
{
    ENGINE_GUARD(e);
    if (!akncp_n || !ncp_n) return fail(ADC_EINVAL, "NULL output");
    if (!e->have_ideal) return fail(ADC_ESTATE, "no ideal profit has been accumulated (adc_engine_ideal_step)");
    if (!e->v.metrics_on) return fail(ADC_ESTATE, "metric mode is off (adc_engine_metrics_enable)");
    if (e->v.K > kMedianMaxK) return fail(ADC_EINVAL, "num_keywords beyond the device-side median (4096): reduce adc_engine_metrics_read_nk on the host");
    const size_t n = (size_t)e->v.N;
    double *d = nullptr;
    if (hipMalloc((void **)&d, 2 * n * 8) != hipSuccess) return fail(ADC_ENOMEM, "hipMalloc failed");
    int P = 1;
    while (P < e->v.K) P <<= 1;
    hipLaunchKernelGGL(k_akncp_ncp, dim3((unsigned)n), dim3(kMedianBlock), (size_t)P * 8, e->stream, e->v, e->pol, days, d, d + n);
    int rc = ADC_OK;
    if (hipGetLastError() != hipSuccess) rc = fail(ADC_EHIP, "k_akncp_ncp launch failed");
    if (!rc && (hipMemcpyAsync(akncp_n, d, n * 8, hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
                hipMemcpyAsync(ncp_n, d + n, n * 8, hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
                hipStreamSynchronize(e->stream) != hipSuccess))
        rc = fail(ADC_EHIP, "download failed");
    (void)hipFree(d);
    return rc;
}

// ---- NaiveInterpolationStrategy, one agent per env (parts/kernel_interp_agent.inc) ---------------------------------------
namespace {
// the agent's view of the env group that starts at env e0: every per-keyword and per-env array moves to that env; the
// slot-major lists keep the engine's stride
inline InterpView interp_view_from(const adc_engine *e, size_t e0)
{
    InterpView p = e->ip;
    const size_t o = e0, ok = o * (size_t)e->v.K;
    auto at = [](auto *&ptr, size_t off) { if (ptr) ptr += off; };
    at(p.ave_rpc, ok); at(p.n_rpc, ok); at(p.ave_sctr, ok); at(p.n_sctr, ok); at(p.max_obs, ok); at(p.last_bid, ok); at(p.last_index, ok);
    at(p.n_clk, ok); at(p.n_cpc, ok); at(p.clk_cent, ok); at(p.clk_ave, ok); at(p.clk_cnt, ok);
    at(p.cpc_cent, ok); at(p.cpc_ave, ok); at(p.cpc_cnt, ok); at(p.kw_cost, ok); at(p.kw_profit, ok);
    at(p.budget, o); at(p.profit, o); at(p.cost, o); at(p.key, o); at(p.tick, o);
    return p;
}
// `more` further updates fit the lists (a capacity of 300 holds every cent)
inline bool interp_room(const adc_engine *e, long long more)
{
    return e->ip.cap >= adc::kInterpCents || e->interp_updates + more <= (long long)e->ip.cap;
}
inline int interp_grid_check(const double *bids, int n)
{
    if (!bids || n < 1 || n > adc::kInterpMaxBids) return fail(ADC_EINVAL, "allowed_bids must hold 1 to 2048 values");
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(bids[i])) return fail(ADC_EINVAL, "allowed_bids must be finite");
    return ADC_OK;
}
int interp_step_chained(adc_engine *e, float budget_override)
{
    if (!e->have_interp) return fail(ADC_ESTATE, "adc_engine_interp_init has not been called");
    // counted before anything is enqueued, so that a launch failing partway leaves the count high, never low (a captured day
    // is counted where its graph is launched)
    if (!e->in_capture) e->interp_updates += 1;
    return launch_chained(e, [&](const View &v, const PolicyView &, hipStream_t st, float *d_bids, float *d_budget) {
        const InterpView p = interp_view_from(e, (size_t)(d_budget - e->d_budget));      // (the group's first env)
        hipLaunchKernelGGL(k_interp_step, dim3((unsigned)v.N), dim3(256), 0, st, v, p, (const float *)nullptr, v.clk, v.cost,
                           v.conv, v.rev, 1, 1, (const double *)nullptr, budget_override, d_bids, d_budget);
    });
}
}  // namespace

ADC_EXPORT int adc_engine_interp_init(adc_engine *e, double threshold, double bid_step, const double *allowed_bids, int32_t n_bids,
                                      int32_t capacity, const uint64_t *seeds_n)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!std::isfinite(threshold) || !std::isfinite(bid_step)) return fail(ADC_EINVAL, "threshold and bid_step must be finite");
    if (int rc = interp_grid_check(allowed_bids, n_bids)) return rc;
    if (capacity < 0 || capacity > adc::kInterpCents) return fail(ADC_EINVAL, "capacity must be 0 (default) to 300");
    ENGINE_GUARD(e);
    const int cap = capacity > 0 ? capacity : std::min(adc::kInterpCents, std::max(1, e->v.max_days + 1));
    const size_t N = e->v.N, nk = N * e->v.K;
    if (e->have_interp && cap != e->ip.cap) return fail(ADC_EINVAL, "the capacity is fixed by the first adc_engine_interp_init");
    if (!e->have_interp) {
        InterpView &p = e->ip;
        const size_t slots = nk * (size_t)cap;
        int rc;
        if ((rc = dev_alloc(e, &p.ave_rpc, nk)) || (rc = dev_alloc(e, &p.n_rpc, nk)) || (rc = dev_alloc(e, &p.ave_sctr, nk)) ||
            (rc = dev_alloc(e, &p.n_sctr, nk)) || (rc = dev_alloc(e, &p.max_obs, nk)) || (rc = dev_alloc(e, &p.last_bid, nk)) ||
            (rc = dev_alloc(e, &p.last_index, nk)) ||
            (rc = dev_alloc(e, &p.n_clk, nk)) || (rc = dev_alloc(e, &p.n_cpc, nk)) || (rc = dev_alloc(e, &p.clk_cent, slots)) ||
            (rc = dev_alloc(e, &p.clk_ave, slots)) || (rc = dev_alloc(e, &p.clk_cnt, slots)) || (rc = dev_alloc(e, &p.cpc_cent, slots)) ||
            (rc = dev_alloc(e, &p.cpc_ave, slots)) || (rc = dev_alloc(e, &p.cpc_cnt, slots)) || (rc = dev_alloc(e, &p.kw_cost, nk)) ||
            (rc = dev_alloc(e, &p.kw_profit, nk)) || (rc = dev_alloc(e, &p.budget, N)) || (rc = dev_alloc(e, &p.profit, N)) ||
            (rc = dev_alloc(e, &p.cost, N)) || (rc = dev_alloc(e, &p.key, N)) || (rc = dev_alloc(e, &p.tick, N)))
            return rc;
        double *grid = nullptr;
        if ((rc = dev_alloc(e, &grid, (size_t)adc::kInterpMaxBids))) return rc;
        p.grid = grid;
        p.cap = cap;
        p.slot_stride = nk;
        e->have_interp = true;
    }
    e->ip.threshold = threshold;
    e->ip.bid_step = bid_step;
    e->ip.n_bids = n_bids;
    HIP_TRY(hipMemcpyAsync(const_cast<double *>(e->ip.grid), allowed_bids, (size_t)n_bids * 8, hipMemcpyHostToDevice, e->stream));
    e->interp_updates = 0;
    uint64_t *d_seeds = nullptr;
    if (seeds_n) { HIP_TRY(hipMalloc((void **)&d_seeds, N * 8)); HIP_TRY(hipMemcpyAsync(d_seeds, seeds_n, N * 8, hipMemcpyHostToDevice, e->stream)); }
    hipLaunchKernelGGL(k_interp_init, dim3((unsigned)((e->v.K + 255) / 256), (unsigned)N), dim3(256), 0, e->stream, e->ip, e->v.K,
                       d_seeds, e->cfg.seed, e->cfg.env_id_base);
    hipError_t err = hipGetLastError();
    hipError_t err2 = hipStreamSynchronize(e->stream);
    if (d_seeds) (void)hipFree(d_seeds);
    HIP_TRY(err);
    HIP_TRY(err2);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_interp_set_allowed_bids(adc_engine *e, const double *bids, int32_t n)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = interp_grid_check(bids, n)) return rc;
    if (!e->have_interp) return fail(ADC_ESTATE, "adc_engine_interp_init has not been called");
    ENGINE_GUARD(e);
    HIP_TRY(hipMemcpyAsync(const_cast<double *>(e->ip.grid), bids, (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->ip.n_bids = n;
    return ADC_OK;
}

namespace {
// update (host arrays: all five or none) and/or act on the engine's stream; host inputs are staged through temporaries
int interp_launch(adc_engine *e, const double *prev_bids_nk, const int32_t *clicks_nk, const float *cost_nk, const int32_t *conv_nk,
                  const float *rev_nk, int do_update, int do_act, const double *replay_u_nk, float budget_override)
{
    const size_t nk = (size_t)e->v.N * e->v.K;
    std::vector<float> bids32;
    if (do_update && prev_bids_nk) {
        bids32.resize(nk);
        for (size_t i = 0; i < nk; ++i) bids32[i] = (float)prev_bids_nk[i];       // torch.Tensor([prev_bid])
    }
    float *d_bid = nullptr, *d_cost = nullptr, *d_rev = nullptr;
    int32_t *d_clk = nullptr, *d_conv = nullptr;
    double *d_u = nullptr;
    auto done = [&](hipError_t err) {
        hipError_t e2 = hipStreamSynchronize(e->stream);
        (void)hipFree(d_bid); (void)hipFree(d_cost); (void)hipFree(d_rev); (void)hipFree(d_clk); (void)hipFree(d_conv); (void)hipFree(d_u);
        if (err != hipSuccess) return fail(ADC_EHIP, hipGetErrorString(err));
        if (e2 != hipSuccess) return fail(ADC_EHIP, hipGetErrorString(e2));
        return (int)ADC_OK;
    };
    hipError_t err = hipSuccess;
    if (do_update && prev_bids_nk) {
        if (hipMalloc((void **)&d_bid, nk * 4) != hipSuccess || hipMalloc((void **)&d_clk, nk * 4) != hipSuccess ||
            hipMalloc((void **)&d_cost, nk * 4) != hipSuccess || hipMalloc((void **)&d_conv, nk * 4) != hipSuccess ||
            hipMalloc((void **)&d_rev, nk * 4) != hipSuccess) { (void)done(hipSuccess); return fail(ADC_ENOMEM, "hipMalloc failed"); }
        err = hipMemcpyAsync(d_bid, bids32.data(), nk * 4, hipMemcpyHostToDevice, e->stream);
        if (err == hipSuccess) err = hipMemcpyAsync(d_clk, clicks_nk, nk * 4, hipMemcpyHostToDevice, e->stream);
        if (err == hipSuccess) err = hipMemcpyAsync(d_cost, cost_nk, nk * 4, hipMemcpyHostToDevice, e->stream);
        if (err == hipSuccess) err = hipMemcpyAsync(d_conv, conv_nk, nk * 4, hipMemcpyHostToDevice, e->stream);
        if (err == hipSuccess) err = hipMemcpyAsync(d_rev, rev_nk, nk * 4, hipMemcpyHostToDevice, e->stream);
    }
    if (err == hipSuccess && replay_u_nk && do_act) {
        if (hipMalloc((void **)&d_u, nk * 8) != hipSuccess) { (void)done(hipSuccess); return fail(ADC_ENOMEM, "hipMalloc failed"); }
        err = hipMemcpyAsync(d_u, replay_u_nk, nk * 8, hipMemcpyHostToDevice, e->stream);
    }
    if (err == hipSuccess) {
        if (do_update) e->interp_updates += 1;        // (before the launch: a failure leaves the count high, never low)
        hipLaunchKernelGGL(k_interp_step, dim3((unsigned)e->v.N), dim3(256), 0, e->stream, e->v, e->ip, (const float *)d_bid,
                           d_clk ? d_clk : e->v.clk, d_cost ? d_cost : e->v.cost, d_conv ? d_conv : e->v.conv, d_rev ? d_rev : e->v.rev,
                           do_update, do_act, (const double *)d_u, budget_override, e->d_bids, e->d_budget);
        err = hipGetLastError();
    }
    return done(err);
}
}  // namespace

ADC_EXPORT int adc_engine_interp_update(adc_engine *e, const double *prev_bids_nk, const int32_t *clicks_nk, const float *cost_nk,
                                        const int32_t *conversions_nk, const float *revenue_nk)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const int given = (prev_bids_nk != nullptr) + (clicks_nk != nullptr) + (cost_nk != nullptr) + (conversions_nk != nullptr) +
                      (revenue_nk != nullptr);
    if (given != 0 && given != 5) return fail(ADC_EINVAL, "pass all of prev_bids/clicks/cost/conversions/revenue, or none");
    if (!e->have_interp) return fail(ADC_ESTATE, "adc_engine_interp_init has not been called");
    if (prev_bids_nk) {
        const size_t nk = (size_t)e->v.N * e->v.K;
        for (size_t i = 0; i < nk; ++i)
            if (!std::isfinite(prev_bids_nk[i])) return fail(ADC_EINVAL, "previous bids must be finite");
    }
    if (!interp_room(e, 1)) return fail(ADC_EINVAL, "the interpolation agent's capacity is full: one more update could overflow it");
    ENGINE_GUARD(e);
    return interp_launch(e, prev_bids_nk, clicks_nk, cost_nk, conversions_nk, revenue_nk, 1, 0, nullptr, 0.0f);
}

ADC_EXPORT int adc_engine_interp_act(adc_engine *e, float budget_override, const double *replay_uniforms_nk)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->have_interp) return fail(ADC_ESTATE, "adc_engine_interp_init has not been called");
    ENGINE_GUARD(e);
    return interp_launch(e, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, replay_uniforms_nk, budget_override);
}

ADC_EXPORT int adc_engine_interp_step(adc_engine *e, float budget_override)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->have_interp) return fail(ADC_ESTATE, "adc_engine_interp_init has not been called");
    if (!interp_room(e, 1)) return fail(ADC_EINVAL, "the interpolation agent's capacity is full: one more update could overflow it");
    ENGINE_GUARD_STEP(e);
    return interp_step_chained(e, budget_override);
}

ADC_EXPORT int adc_engine_interp_state(adc_engine *e, float *ave_rpc_nk, int32_t *num_rpc_obs_nk, float *ave_sctr_nk,
                                       int32_t *num_sctr_obs_nk, double *max_observed_nk, int32_t *bid_index_nk, double *budget_n, double *profit_beliefs_n,
                                       double *cost_beliefs_n)
{
    ENGINE_GUARD(e);
    if (!e->have_interp) return fail(ADC_ESTATE, "adc_engine_interp_init has not been called");
    const size_t n = (size_t)e->v.N, nk = n * e->v.K;
    const InterpView &p = e->ip;
    if (ave_rpc_nk) HIP_TRY(hipMemcpyAsync(ave_rpc_nk, p.ave_rpc, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (num_rpc_obs_nk) HIP_TRY(hipMemcpyAsync(num_rpc_obs_nk, p.n_rpc, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (ave_sctr_nk) HIP_TRY(hipMemcpyAsync(ave_sctr_nk, p.ave_sctr, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (num_sctr_obs_nk) HIP_TRY(hipMemcpyAsync(num_sctr_obs_nk, p.n_sctr, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (max_observed_nk) HIP_TRY(hipMemcpyAsync(max_observed_nk, p.max_obs, nk * 8, hipMemcpyDeviceToHost, e->stream));
    if (bid_index_nk) HIP_TRY(hipMemcpyAsync(bid_index_nk, p.last_index, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (budget_n) HIP_TRY(hipMemcpyAsync(budget_n, p.budget, n * 8, hipMemcpyDeviceToHost, e->stream));
    if (profit_beliefs_n) HIP_TRY(hipMemcpyAsync(profit_beliefs_n, p.profit, n * 8, hipMemcpyDeviceToHost, e->stream));
    if (cost_beliefs_n) HIP_TRY(hipMemcpyAsync(cost_beliefs_n, p.cost, n * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_interp_entries(adc_engine *e, int32_t *capacity, int32_t *n_clicks_nk, uint16_t *clicks_cent_cnk,
                                         float *ave_clicks_cnk, int32_t *clicks_count_cnk, int32_t *n_cpc_nk, uint16_t *cpc_cent_cnk,
                                         double *ave_cpc_cnk, int32_t *cpc_count_cnk)
{
    ENGINE_GUARD(e);
    if (!e->have_interp) return fail(ADC_ESTATE, "adc_engine_interp_init has not been called");
    const InterpView &p = e->ip;
    const size_t nk = (size_t)e->v.N * e->v.K, slots = nk * (size_t)p.cap;
    if (capacity) *capacity = p.cap;
    if (n_clicks_nk) HIP_TRY(hipMemcpyAsync(n_clicks_nk, p.n_clk, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (clicks_cent_cnk) HIP_TRY(hipMemcpyAsync(clicks_cent_cnk, p.clk_cent, slots * 2, hipMemcpyDeviceToHost, e->stream));
    if (ave_clicks_cnk) HIP_TRY(hipMemcpyAsync(ave_clicks_cnk, p.clk_ave, slots * 4, hipMemcpyDeviceToHost, e->stream));
    if (clicks_count_cnk) HIP_TRY(hipMemcpyAsync(clicks_count_cnk, p.clk_cnt, slots * 4, hipMemcpyDeviceToHost, e->stream));
    if (n_cpc_nk) HIP_TRY(hipMemcpyAsync(n_cpc_nk, p.n_cpc, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (cpc_cent_cnk) HIP_TRY(hipMemcpyAsync(cpc_cent_cnk, p.cpc_cent, slots * 2, hipMemcpyDeviceToHost, e->stream));
    if (ave_cpc_cnk) HIP_TRY(hipMemcpyAsync(ave_cpc_cnk, p.cpc_ave, slots * 8, hipMemcpyDeviceToHost, e->stream));
    if (cpc_count_cnk) HIP_TRY(hipMemcpyAsync(cpc_count_cnk, p.cpc_cnt, slots * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

#ifdef ADC_EXP_TIMING
extern "C" __attribute__((visibility("default"))) int adc_debug_read(unsigned long long *out, int reset)
{
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dbg), sizeof(unsigned long long) * 16);
    // slots 8..15: k_step_implicit_fast (wave 0 of every workgroup), summed over the 256 rows of g_fdbg
    static unsigned long long rows[256][8];
    hipMemcpyFromSymbol(rows, HIP_SYMBOL(g_fdbg), sizeof(rows));
    for (int i = 0; i < 8; ++i) { out[8 + i] = 0; for (int r = 0; r < 256; ++r) out[8 + i] += rows[r][i]; }
    if (reset) {
        unsigned long long z[16] = {0};
        hipMemcpyToSymbol(HIP_SYMBOL(g_dbg), z, sizeof(z));
        std::memset(rows, 0, sizeof(rows));
        hipMemcpyToSymbol(HIP_SYMBOL(g_fdbg), rows, sizeof(rows));
    }
    return 0;
}

// k_step_implicit_fast, all waves since the last reset: out2 = {Philox calls issued in phase 2 (wave-call-slots), calls that hold at
// least one auction (lane-calls: 64 of them fill a slot)}
extern "C" __attribute__((visibility("default"))) int adc_debug_read_fast_slots(unsigned long long *out2, int reset)
{
    hipDeviceSynchronize();
    static unsigned long long rows[256][2];
    hipMemcpyFromSymbol(rows, HIP_SYMBOL(g_fslots), sizeof(rows));
    out2[0] = out2[1] = 0;
    for (int r = 0; r < 256; ++r) { out2[0] += rows[r][0]; out2[1] += rows[r][1]; }
    if (reset) {
        std::memset(rows, 0, sizeof(rows));
        hipMemcpyToSymbol(HIP_SYMBOL(g_fslots), rows, sizeof(rows));
    }
    return 0;
}
#endif
