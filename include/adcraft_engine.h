/*
 * adcraft_engine.h - C ABI of the MI355X-native vectorised BiddingSimulation step engine.
 *
 * This is the drop-in boundary for the reference's per-step hot path.  The reference crosses
 * its native boundary through the pyo3 module `adcraft.rust` (src/lib.rs:14-15,
 * pyproject.toml:38-40) ~10 times per (sub-timestep, keyword) from
 * adcraft/bidding_simulation.py:44-234 and adcraft/gymnasium_kw_env.py:160-269.  A replacement
 * binds ONE call per step for ALL environments instead (adc_engine_step*), plus the scalar
 * entry points that mirror `adcraft.rust` one-to-one for callers that still want them.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch/Python types.
 *   - every function returns ADC_OK (0) or a negative adc_status; adc_last_error() returns a
 *     thread-local message for the last failure on the calling thread.
 *   - host buffers are caller-allocated and only borrowed for the duration of the call; device
 *     state is owned by the engine handle; adc_engine_destroy frees it.
 *   - an engine handle is not thread-safe (one caller at a time, like a gym env); different
 *     handles are independent.  ctypes releases the GIL during calls.
 *   - there is NO CPU backend: with no usable HIP device adc_engine_create fails with ADC_EHIP.
 *
 * Layout: all per-keyword arrays are [num_envs][num_keywords], keyword fastest (row-major),
 * parameter planes are [ADC_P_COUNT][num_envs][num_keywords].
 */
#ifndef ADCRAFT_ENGINE_H
#define ADCRAFT_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADC_ABI_VERSION 5
/* revision of the engine's own random stream (which variate lives at which Philox counter): results under a
 * fixed seed - and golden streams recorded from an engine - are comparable only between libraries of the same revision.
 * 2: IMPLICIT / EXPLICIT layout since round 2; 3, 4: IMPLICIT_GENERAL top bids as order statistics, bidder count by inversion;
 * 5: the competitor bids the ideal-profit estimator samples (stage METRIC) by the auction law's own transform of a word (the step's
 *    own streams are those of revision 4) */
#define ADC_STREAM_REVISION 5

typedef enum adc_status {
    ADC_OK = 0,
    ADC_EINVAL = -1,   /* bad argument (-> ValueError / AssertionError in the Python host layer) */
    ADC_EHIP = -2,     /* HIP runtime failure or no device (-> RuntimeError) */
    ADC_ENOMEM = -3,   /* device or host allocation failed (-> MemoryError) */
    ADC_ESTATE = -4,   /* call not valid in the current state, e.g. step before reset */
    ADC_ETYPE = -5,    /* wrong element type for a reducer shim (-> TypeError, see adcraft.rust tests) */
    ADC_ERCCL = -6     /* librccl missing, or an RCCL call of the metric all-reduce failed (-> RuntimeError) */
} adc_status;

/* keyword model: which of the reference's two Keyword subclasses the engine simulates */
typedef enum adc_model {
    ADC_MODEL_IMPLICIT = 0,  /* ImplicitKeyword: literal 2nd-price auction vs one sampled competitor bid
                                (adcraft/synthetic_kw_classes.py:578-646, gymnasium_kw_utils.py:169-195) */
    ADC_MODEL_EXPLICIT = 1,  /* ExplicitKeyword: sigmoid impression rate + Binomial + parametric cost
                                (adcraft/synthetic_kw_classes.py:457-575, gymnasium_kw_utils.py:67-96) */
    ADC_MODEL_IMPLICIT_GENERAL = 2   /* the DEFAULT ImplicitKeyword (not the env's single-competitor form): B ~ Binomial(max_bidders,
                                participation_rate) bidders drawn once per (sub-timestep, keyword) call, raw Laplace(loc, scale) bids,
                                the literal top-(w+n) clearing of nth_price_auction with n = 2: won iff the bid exceeds the (w)-th
                                highest competitor bid, price = the bid just below ours; float64 money
                                (adcraft/synthetic_kw_classes.py:610-686, adcraft/synthetic_kw_helpers.py:116-180).
                                Parameter planes A / B = bid_loc / bid_scale; pool and winners: adc_engine_set_general_model */
} adc_model;

/* parameter planes (float32).  Slots 2,3 depend on the model. */
typedef enum adc_param {
    ADC_P_VOL_MEAN = 0,   /* volume ~ round(max(N(mean, std), 0)), src/lib.rs:314-325 */
    ADC_P_VOL_STD = 1,
    ADC_P_A = 2,          /* IMPLICIT: competitor-bid Laplace loc   | EXPLICIT: impression_bid_intercept */
    ADC_P_B = 3,          /* IMPLICIT: competitor-bid Laplace scale | EXPLICIT: impression_slope */
    ADC_P_BCTR = 4,       /* buyside_ctr */
    ADC_P_SCTR = 5,       /* sellside_paid_ctr */
    ADC_P_REV_MEAN = 6,   /* revenue ~ round2(max(N(mean, std), 0.01)), synthetic_kw_helpers.py:66-70 */
    ADC_P_REV_STD = 7,
    ADC_P_COUNT = 8
} adc_param;

typedef struct adc_config {
    uint32_t struct_size;      /* sizeof(adc_config), for forward compatibility */
    int32_t device_id;         /* HIP device ordinal */
    int32_t num_envs;          /* environments resident on this device */
    int32_t num_keywords;      /* keywords per environment (BiddingSimulation.num_keywords) */
    int32_t model;             /* adc_model */
    int32_t max_days;          /* gymnasium_kw_env.py:61,228 */
    double loss_threshold;     /* dollars; gymnasium_kw_env.py:60,225 */
    float drift_vol;           /* updater_params [["vol",a],["ctr",b],["cvr",c]], gymnasium_kw_env.py:62 */
    float drift_ctr;
    float drift_cvr;
    int32_t drift_enabled;     /* updater_mask == [True]*K (the only mask the reference's configs use) */
    float impression_thresh;   /* EXPLICIT: impression_thresh, 0.05 in the env (gymnasium_kw_utils.py:81) */
    int32_t auto_reset;        /* vector form: a finished env restarts (day=0, cum=0) after reporting */
    int64_t env_id_base;       /* global id of local env 0 (multi-GPU sharding; used for default keys) */
    uint64_t seed;             /* engine seed; env e gets key = mix(seed, env_id_base + e) until reset with a seed */
} adc_config;

/* caller-allocated host outputs of one step; any pointer may be NULL to skip that copy */
typedef struct adc_step_out {
    int32_t *impressions;      /* [N*K] obs["impressions"] */
    int32_t *buyside_clicks;   /* [N*K] obs["buyside_clicks"] */
    int32_t *sellside_conversions; /* [N*K] */
    float *cost;               /* [N*K] dollars, obs["cost"] */
    float *revenue;            /* [N*K] dollars, obs["revenue"] */
    double *reward;            /* [N]   step profit, gymnasium_kw_env.py:222,230 */
    double *cumulative_profit; /* [N]   after the step, :223,242 */
    int32_t *days_passed;      /* [N]   after the step, :227,243 */
    uint8_t *terminated;       /* [N]   :228 */
    uint8_t *truncated;        /* [N]   :225 */
    /* optional compact form of the three counts: uint16 [N][3][K] = per env: impressions | buyside_clicks |
     * sellside_conversions (K even), packed on the device: 6 B instead of 12 B per keyword over PCIe (a host step of
     * 4096 x 256 is PCIe-bound).  A count above 65535 is stored as 65535 and *counts_overflow (nullable) is set to 1:
     * use the int32 pointers then. */
    uint16_t *counts_u16;
    int32_t *counts_overflow;
} adc_step_out;

/* device-resident buffers of the engine (for zero-copy consumers: torch / DLPack / RL on GPU) */
typedef enum adc_buffer {
    ADC_BUF_PARAMS = 0,        /* float [8][N][K] */
    ADC_BUF_BIDS = 1,          /* float [N][K]  engine-owned action staging buffer */
    ADC_BUF_BUDGET = 2,        /* float [N] */
    ADC_BUF_IMPRESSIONS = 3,   /* int32 [N][K] */
    ADC_BUF_CLICKS = 4,
    ADC_BUF_CONVERSIONS = 5,
    ADC_BUF_COST = 6,          /* float [N][K] */
    ADC_BUF_REVENUE = 7,
    ADC_BUF_REWARD = 8,        /* double [N] */
    ADC_BUF_CUM_PROFIT = 9,    /* double [N] */
    ADC_BUF_DAYS = 10,         /* int32 [N] */
    ADC_BUF_TERMINATED = 11,   /* uint8 [N] */
    ADC_BUF_TRUNCATED = 12,
    ADC_BUF_METRIC_PROFIT = 13,/* int64 [K]  sum over local envs and steps of keyword profit, cents (valid after metrics_read) */
    ADC_BUF_METRIC_SCALARS = 14,/* int64 [8]  {profit_cents, env_steps, episodes, truncations, auctions, 0,0,0} */
    ADC_BUF_FLAT_OBS = 15,     /* float [N][5K+2] FlatArrayWrapper layout (adcraft/wrappers/flat_array.py:74-80) */
    /* the rollout record of the MLP policy (adc_engine_rollout_enable), horizon T, A = K + 1, D = 5K + 2 */
    ADC_BUF_ROLLOUT_ACTION = 16,    /* float [T][N][A] unclipped actions, flat action order [budget, bids...] */
    ADC_BUF_ROLLOUT_LOGP = 17,      /* float [T][N] */
    ADC_BUF_ROLLOUT_VALUE = 18,     /* float [T][N] */
    ADC_BUF_ROLLOUT_REWARD = 19,    /* float [T][N] */
    ADC_BUF_ROLLOUT_TERMINATED = 20,/* uint8 [T][N] */
    ADC_BUF_ROLLOUT_TRUNCATED = 21, /* uint8 [T][N] */
    ADC_BUF_ROLLOUT_OBS = 22        /* float [T][N][D] the (normalised) network input; only with ADC_ROLLOUT_OBS */
} adc_buffer;

/* replay ("tape") variate source: the variates the reference drew, in the order it drew them
 * (t-major, keyword-minor; adcraft/bidding_simulation.py:216-233).  Used for bit-exact parity
 * against fixtures recorded from the reference.  Per-env start offsets index the flat tapes;
 * `*_end` (nullable, [N]) receives the cursor after the step. */
typedef struct adc_tape {
    const int32_t *volumes;        /* [N*K] auction volume of each keyword this step */
    const int32_t *bid_cents;      /* IMPLICIT: competitor bids in cents, n per visited cell */
    const int32_t *x_impressions;  /* EXPLICIT: Binomial result per visited cell; IMPLICIT_GENERAL: bidders of the cell */
    const double *x_cost;          /* EXPLICIT: per-impression costs; IMPLICIT_GENERAL: bids, bidders x auctions per cell (bidder-major) */
    const uint8_t *click;          /* one per won auction (IMPLICIT) / per cost entry incl. phantom (EXPLICIT) */
    const uint8_t *conv;           /* one per paid click */
    const int32_t *rev_cents;      /* one per conversion */
    int64_t len_bid, len_ximp, len_xcost, len_click, len_conv, len_rev;  /* tape lengths (bounds checks) */
    const int64_t *off_bid, *off_ximp, *off_xcost, *off_click, *off_conv, *off_rev;   /* [N] start cursors */
    int64_t *end_bid, *end_ximp, *end_xcost, *end_click, *end_conv, *end_rev;         /* [N] nullable */
    /* nullable [3][N*K]: the three coefficient vectors update_keywords() drew, np_random.uniform(-a, a, size=K) in its
     * order vol, ctr, cvr (adcraft/gymnasium_kw_env.py:132-135).  When given (drift must be enabled) the replayed step ends
     * with update_keywords() on exactly these coefficients (:246), applied at once instead of from the engine's stream. */
    const float *drift_uniforms;
} adc_tape;

/* quantile tables for device-side keyword generation: the rows of the reference's quantile DataFrame, per quantity
 * (order: vol, ave_cpc, std_cpc, bctr, sctr, rpsc, std_rpsc), already filtered to count_<param> > 0
 * (adcraft/gymnasium_kw_utils.py:296-332) */
typedef struct adc_quantiles {
    int32_t buckets[7];
    const float *mins[7], *medians[7], *maxs[7];     /* [buckets[i]] each */
} adc_quantiles;

typedef struct adc_engine adc_engine;

/* ---- lifecycle ---------------------------------------------------------------------------------- */
int adc_abi_version(void);
int adc_stream_revision(void);
const char *adc_last_error(void);
int adc_device_count(int *count);
int adc_engine_create(const adc_config *cfg, adc_engine **out);
void adc_engine_destroy(adc_engine *e);

/* ---- keyword state (what reset() generates host-side: gymnasium_kw_env.py:303-316) --------------- */
/* one parameter plane for all envs, host float [N*K] */
int adc_engine_set_params(adc_engine *e, int param_id, const float *host_nk);
int adc_engine_get_params(adc_engine *e, int param_id, float *host_nk);   /* applies pending drift first */
/* all 8 planes of ONE env, host float [8][K] */
int adc_engine_set_env_params(adc_engine *e, int env, const float *host_8k);

/* draw the keyword set of every env with env_mask[e]!=0 (NULL = all) on the device: the law of
 * sample_implicit_keywords_from_quantile_dfs (gymnasium_kw_utils.py:295-339: bucket pick + piecewise-linear
 * interpolation, no_vol_prob, std un-normalisation), from the env's own Philox key (call after a reset with seeds);
 * `serial` distinguishes successive generations under the same key (0 right after a seeded reset, so that the same
 * seed reproduces the same keyword set).
 * Same law as the host recipe, NOT the same numbers as the reference's PCG64 draws (those are reproduced by
 * generating host-side and uploading with adc_engine_set_params). */
int adc_engine_generate_keywords(adc_engine *e, const adc_quantiles *q, float no_vol_prob, uint32_t serial,
                                 const uint8_t *env_mask);

/* the same for the EXPLICIT model (the default constructor's keyword set): the law of sample_random_keywords
 * (gymnasium_kw_utils.py:113-156, draws :129-140) - vol_mean = int(2^Beta(2,5) 15 - 1), vol_std = U 0.5 (vol_mean + 1),
 * sctr ~ Beta(5,2), intercept = 1.5 U, rev_mean = 1.5 Beta(2,5), rev_std = Beta(2,5) rev_mean, bctr ~ Beta(2,5),
 * slope = 25 Beta(5,5) - from the env's own Philox key; every Beta is an order statistic of uniforms (integer parameters: exact).
 * Same law, not the reference's PCG64 numbers (those: sample host-side, adc_engine_set_params). */
int adc_engine_generate_explicit_keywords(adc_engine *e, uint32_t serial, const uint8_t *env_mask);

/* reset(): day=0, cumulative_profit=0 for envs with env_mask[e]!=0 (NULL = all);
 * seeds (nullable, [N]) re-key the env's random stream (reset(seed=...)); gymnasium_kw_env.py:271-346 */
int adc_engine_reset(adc_engine *e, const uint8_t *env_mask, const uint64_t *seeds);

/* reset(options={"max_days":..., "loss_threshold":...}) and set_updater_mask()/updater_params changes
 * (gymnasium_kw_env.py:105-112,318-325) */
int adc_engine_set_limits(adc_engine *e, int32_t max_days, double loss_threshold);
int adc_engine_set_drift(adc_engine *e, int32_t enabled, float drift_vol, float drift_ctr, float drift_cvr);
/* which keywords drift at each update_keywords(), per env: mask_nk[N][K] (nonzero = moves), NULL = every keyword.
 * A selected keyword moves exactly as without a selection (same draw, same magnitudes); an unselected one keeps vol_mean,
 * bctr and sctr bit for bit.  An explicit selection: the reference's prefix rule for a partial updater_mask
 * (gymnasium_kw_env.py:130-144, keyword k moves iff mask[k] and k < sum(mask)) is the caller's to apply.
 * The update the last step scheduled is first applied under the selection in force when it was scheduled.
 * Persists across resets; does not switch drift on (adc_engine_set_drift does). */
int adc_engine_set_drift_mask(adc_engine *e, const uint8_t *mask_nk);
/* per-env drift magnitudes rates_n3[N][3] = vol, ctr, cvr (updater_params' numbers), NULL = adc_engine_set_drift's scalars.
 * While set they override those scalars (adc_engine_set_drift still switches drift on and off).  The pending update is first
 * applied under the magnitudes in force when it was scheduled.  Persists across resets. */
int adc_engine_set_env_drift(adc_engine *e, const float *rates_n3);

/* random-stream state of every env: Philox key [N] and step counter ("tick") [N]; with the episode state
 * below this is everything needed to checkpoint / resume an engine (the parameters come from get_params) */
int adc_engine_get_rng_state(adc_engine *e, uint64_t *keys_n, uint32_t *ticks_n);
int adc_engine_set_rng_state(adc_engine *e, const uint64_t *keys_n, const uint32_t *ticks_n);
/* episode state: current_day [N], cumulative_profit in dollars [N] (gymnasium_kw_env.py:327-328) */
int adc_engine_get_episode_state(adc_engine *e, int32_t *day_n, double *cum_profit_n);
int adc_engine_set_episode_state(adc_engine *e, const int32_t *day_n, const double *cum_profit_n);

/* ---- the hot path: BiddingSimulation.step for all envs (gymnasium_kw_env.py:160-269) ------------- */
/* host in / host out, synchronous.  bids [N*K] (action["keyword_bids"]), budget [N] (action["budget"]). */
int adc_engine_step(adc_engine *e, const float *bids_nk, const float *budget_n, adc_step_out *out);
/* device in / device out, asynchronous on the engine's stream (NULL = use the engine's staging buffers) */
int adc_engine_step_device(adc_engine *e, const float *d_bids_nk, const float *d_budget_n);
/* copy the last step's outputs to host buffers (synchronises) */
int adc_engine_fetch(adc_engine *e, adc_step_out *out);
/* Byte offsets of the ten adc_step_out arrays (in the struct's order) inside the engine's device output block, and the
 * block's size.  Host buffers placed at these offsets of one allocation are filled by ONE transfer; equal-sized outputs at
 * a constant host stride (e.g. planes of one [5][N][K] array) by one 2-D transfer; anything else by one transfer each. */
int adc_engine_out_offsets(const adc_engine *e, size_t offsets[10], size_t *block_bytes);
int adc_engine_synchronize(adc_engine *e);
/* the same step with FlatArrayWrapper-layout host I/O (adcraft/wrappers/flat_array.py:44-87), synchronous:
 * flat_actions [N][K+1] = [budget, bids...] in; flat_obs [N][5K+2] (sorted-key order, see
 * adc_engine_flat_obs_enable) out; reward [N], terminated [N], truncated [N] out (nullable).  The un/flattening
 * happens on the device, so the host moves one array each way. */
int adc_engine_step_flat(adc_engine *e, const float *flat_actions, float *flat_obs, double *reward, uint8_t *terminated,
                         uint8_t *truncated);
/* the asynchronous forms: enqueue (actions up, kernels, outputs down) on the engine's stream and return; adc_engine_wait
 * completes them.  Give them page-locked buffers (adc_host_alloc) and the transfers of one engine overlap the kernels of
 * another on the same device: a vector env split over a few engines hides most of its PCIe time that way. */
int adc_engine_step_async(adc_engine *e, const float *bids_nk, const float *budget_n, adc_step_out *out);
int adc_engine_step_flat_async(adc_engine *e, const float *flat_actions_n_k1, float *flat_obs_n_5k2, double *reward_n,
                               uint8_t *terminated_n, uint8_t *truncated_n);
int adc_engine_wait(adc_engine *e);
/* replay a recorded tape instead of the engine's own random stream (parity mode) */
int adc_engine_step_replay(adc_engine *e, const float *bids_nk, const float *budget_n, const adc_tape *tape,
                           adc_step_out *out);
/* ADC_MODEL_IMPLICIT_GENERAL: the bidder pool (ImplicitKeyword._bidder_distribution_init defaults 30, 0.6) and the number of
 * winning placements (ImplicitKeyword.auction's n_winners, default 1); max_bidders in [0, 252], num_winners in {1, 2} */
int adc_engine_set_general_model(adc_engine *e, int32_t max_bidders, float participation_rate, int32_t num_winners);
/* BiddingSimulation.update_keywords() called directly (gymnasium_kw_env.py:114-158) */
int adc_engine_update_keywords(adc_engine *e);

/* page-locked host memory for step I/O buffers (DMA straight to/from the caller's arrays instead of staged
 * pageable copies); plain malloc-style ownership: free with adc_host_free */
int adc_host_alloc(size_t bytes, void **out);
void adc_host_free(void *p);

/* ---- device-resident access ---------------------------------------------------------------------- */
int adc_engine_device_buffer(adc_engine *e, int buffer_id, void **dptr, size_t *bytes);
int adc_engine_stream(adc_engine *e, void **hip_stream);
/* fill the engine's action staging buffers with synthetic actions: bid = round2(U(lo,hi)) from the
 * engine's ACTION stream at the current tick, budget = `budget` for every env */
int adc_engine_sample_actions(adc_engine *e, float bid_lo, float bid_hi, float budget);
/* emit FlatArrayWrapper-compatible observations [N][5K+2] float32 on the device after every step
 * (sorted-key order: buyside_clicks, cost, cumulative_profit, days_passed, impressions, revenue,
 * sellside_conversions; adcraft/wrappers/flat_array.py:74-80).  Read it through ADC_BUF_FLAT_OBS. */
int adc_engine_flat_obs_enable(adc_engine *e, int enabled);
/* FlatArrayWrapper-compatible action [N][K+1] = [budget, bids...] (device pointer) -> staging buffers */
int adc_engine_set_flat_actions_device(adc_engine *e, const float *d_flat_n_k1);

/* ---- measurement --------------------------------------------------------------------------------- */
/* when enabled, the kernels of every step are bracketed by HIP events on the engine stream */
int adc_engine_profile_enable(adc_engine *e, int enabled);
/* bracket only every `every`-th step (default 1: all).  Recording four events a step keeps a step's small kernels from
 * overlapping the next step's launch - about 16 us per step at 0.21 ms; a sampled measurement leaves the throughput alone. */
int adc_engine_profile_sample_every(adc_engine *e, int32_t every);
/* kernel_ms_total[3] = summed durations of {fast pass, exact pass + step tail, metric accumulate} over `launches`
 * MEASURED steps since enable / the last read; resets the counters */
int adc_engine_profile_read(adc_engine *e, double *kernel_ms_total, int64_t *launches);
/* hipEventRecord calls the engine has issued since it was created (four per bracketed step): lets a benchmark show that
 * its timed region recorded none */
int adc_engine_profile_records(adc_engine *e, int64_t *event_records);
/* GPU time of a whole region of the engine's stream from ONE event pair (nothing per step): `begin` records an event, `end`
 * records another, waits for it and returns the milliseconds between the two - the figure a host-clock timing of K steps is
 * checked against */
int adc_engine_region_begin(adc_engine *e);
int adc_engine_region_end(adc_engine *e, double *gpu_ms);
/* how many ENV GROUPS the last step ran as (1: all envs as one launch per kernel on the engine's stream).  A CHAIN of device-resident
 * steps - adc_engine_step_device following adc_engine_step_device, with nothing between them but the device-side calls that touch
 * every env on its own: adc_engine_agent_step, adc_engine_ideal_step without host outputs, adc_engine_policy_oracle,
 * adc_engine_sample_actions; adc_engine_run_days is such a chain - of an engine with 2048 envs or more (up to 1024 keywords; not the
 * default ImplicitKeyword beyond 512 keywords, nor a budget-free IMPLICIT batch of 16 rounds of workgroups or more, which measured
 * slower) runs as 4 contiguous env groups (2 for sparse IMPLICIT keyword sets), each with its own view of the engine's arrays, its
 * own lists and its own HIP stream: the tail of one group's launch and its small latency-bound kernels (step tail, budget-exact
 * kernels, the per-step ideal) run under another group's keyword-parallel pass, and a group starts its next day while another
 * finishes this one.  Scheduling only - results never depend on it.  Any other call ends the chain: it first makes the engine's
 * stream wait for the groups, so callers order their work behind a step exactly as before, and the step behind it runs as one group
 * (forking and joining the groups costs more than the overlap inside a single step returns).  After adc_engine_stream has handed the
 * stream out, and while profiling brackets kernels with events, every step is one group.  The first grouped step of an engine picks
 * the groups' streams - one per hardware queue, found by a 150 us spin kernel on pairs of candidate streams, because two groups on
 * one queue would run one after the other: 15 to 50 ms, once. */
int adc_engine_env_groups(adc_engine *e, int32_t *groups);
/* ... and fixes it: 0 = the engine chooses (the default), 1..4 = that many groups (capped by the env count; 1 is the one-stream
 * schedule of earlier ABI versions).  ADCRAFT_STREAM_GROUPS in the environment sets the same thing at creation. */
int adc_engine_set_env_groups(adc_engine *e, int32_t groups);
/* name of the kernel the last step's first pass ran (the one kernel_ms_total[0] times).  IMPLICIT: "k_step_implicit_fast<false>"
 * (dense keyword sets, 256 keywords per workgroup), "k_step_implicit_fast<true>" (a handful of envs: narrow tiles), either with
 * ", lists" before the ">" once an env lists its clicked wins for k_step_click_walk ("k_step_implicit_fast<false, lists>"),
 * "k_step_implicit_sparse" (few auctions per keyword); IMPLICIT_GENERAL: "k_step_general_fast", "k_step_general_small" (a handful
 * of envs: a wavefront per keyword); EXPLICIT: "k_step_explicit_fast"; "k_step_exact" after a tape replay; "" before the first
 * step.  A static string: do not free. */
const char *adc_engine_step_kernel_name(adc_engine *e);

/* ---- multi-GPU: the one collective of the path ----------------------------------------------- */
/* Envs shard over the GPUs of a node, one process (one engine) per GPU; nothing on the step path communicates.  The
 * episode-level metric (compute_AKNCP / compute_NCP, adcraft/experiment_utils/experiment_metrics.py:64-83) needs sums over
 * ALL envs: one RCCL all-reduce (sum) of 3K + 8 doubles on the engine's stream, over xGMI.
 *   rank 0:      adc_comm_get_unique_id(id)  and hands the 128 bytes to the other ranks (file, socket, ... - caller's choice)
 *   every rank:  adc_engine_comm_init(engine, id, rank, world_size)         (collective)
 *   per report:  adc_engine_metrics_allreduce(engine, ...)                  (collective)
 * Without a communicator (a single GPU) the calls return the local sums.  librccl.so is opened on first use. */
#define ADC_COMM_ID_BYTES 128
int adc_comm_get_unique_id(uint8_t *id_bytes /* [ADC_COMM_ID_BYTES] */);
int adc_engine_comm_init(adc_engine *e, const uint8_t *id_bytes, int32_t rank, int32_t world_size);
int adc_engine_comm_destroy(adc_engine *e);
int adc_engine_comm_info(adc_engine *e, int32_t *rank, int32_t *world_size);
/* out_3k8[0..K) = keyword profit in cents, [K..2K) = ideal profit, [2K..3K) = ideal profit with <= 0 -> 1 per entry (the
 * denominator compute_AKNCP uses, :71-75), [3K..3K+8) = {profit_cents, env_steps, episodes, truncations, ...}: sums over
 * steps, envs and ranks.  The ideal sums are the engine's own (adc_engine_ideal_step) when it accumulates them; otherwise
 * this rank's contribution may be passed as host vectors ideal_k / ideal_pos_k ([K] doubles each, NULL = zeros). */
int adc_engine_metrics_allreduce(adc_engine *e, const double *ideal_k, const double *ideal_pos_k, double *out_3k8);
/* what the metric reductions have cost on the device so far: calls of adc_engine_metrics_allreduce and the milliseconds (HIP events
 * on the engine's stream, three records per call) of this rank's own reduction kernels and of the ncclAllReduce (0 without a
 * communicator); reset != 0 zeroes the counters afterwards.  Any pointer may be NULL. */
int adc_engine_comm_stats(adc_engine *e, int64_t *calls, double *ms_local_reduction, double *ms_allreduce, int reset);
/* sum (op 0) or max (op 1) of `count` host doubles over the ranks, in place (a barrier is count = 1) */
int adc_engine_comm_allreduce_f64(adc_engine *e, double *inout, int32_t count, int32_t op);

/* ---- episode metrics (adcraft/experiment_utils/experiment_metrics.py:64-83) ----------------------- */
int adc_engine_metrics_enable(adc_engine *e, int enabled);
int adc_engine_metrics_reset(adc_engine *e);
/* local (this device) accumulators to host: keyword_profit_cents [K], scalars [8] */
int adc_engine_metrics_read(adc_engine *e, int64_t *keyword_profit_cents_k, int64_t *scalars8);
/* ideal (max expected) profit per keyword from the CURRENT parameters, n_samples sampled competitor bids and a
 * bid grid in dollars (the notebooks use np.arange(0.01, 3.00, 0.01)); experiment_metrics.py:20-61;
 * host double [N*K].  IMPLICIT keywords: n_samples <= 2^20; every bid finite and at most $20.46 (2046 cents; any order, a bid
 * of 0 or less takes no sample) - otherwise ADC_EINVAL, never a clamped bid.  EXPLICIT keywords: the curves of adc_engine_bid_curves_build (get_explicit_kw_bid_cpc_impressions,
 * experiment_metrics.py:10-17), n_samples <= 2^20.  IMPLICIT_GENERAL: ADC_EINVAL (the reference's estimator on a bidder
 * pool gives impression rates above 1). */
int adc_engine_ideal_profit(adc_engine *e, int n_samples, const double *bid_grid, int n_bids, double *host_nk);
/* the estimator alone, on caller-supplied competitor-bid samples (cents) of one keyword: impression rate and
 * expected cpc on the given bid grid, exactly as get_implicit_kw_bid_cpc_impressions computes them
 * (experiment_metrics.py:28-37, including its inclusive running-mean index).  Samples >= 0, n_samples <= 2^20 and the IMPLICIT
 * grid limits of adc_engine_ideal_profit, all checked before any HIP call (ADC_EINVAL). */
int adc_bid_curves_from_samples(int device_id, const int32_t *samples_cents, int32_t n_samples, const double *bid_grid,
                                int32_t n_bids, double *impression_rate_out, double *cpc_out);

/* ---- the callers of the step, device-resident: per-step ideal profit and the paper's baseline bidders ----------
 * (the loop of adcraft/baseline_experiment_and_figs_notebooks/run_heatmap_experiments.ipynb cell 1 and
 * timing_and_other_one_off_experiments.ipynb cell 2: agent.update_all_caches -> agent.sample_action ->
 * get_max_expected_bid_profits per keyword -> env.step -> profits).  All of it runs on the engine's stream against the
 * engine's device-resident observation and action buffers: no host round trip per step. */

/* impression-rate / expected-cpc curves of every keyword on `bid_grid` from n_samples sampled competitor bids
 * (get_implicit_kw_bid_cpc_impressions, experiment_metrics.py:20-37; the notebooks build them once after reset()).
 * Kept on the device as integer numerators, 8 bytes x N x K x n_bids; n_samples <= 2^20, bids as for adc_engine_ideal_profit.
 * EXPLICIT keywords: get_explicit_kw_bid_cpc_impressions (:10-17) - impression rate = threshold_sigmoid, cpc = the median of
 * n_samples costs, drawn once per keyword (the grid's bids share the draws) and kept as the two middle normals with the
 * impression intercept and slope: 16 bytes x N x K, plus 24 bytes per grid point.  IMPLICIT_GENERAL: ADC_EINVAL. */
int adc_engine_bid_curves_build(adc_engine *e, int n_samples, const double *bid_grid, int n_bids);
/* the cached curves to host: impression rate and expected cpc, double [N*K][n_bids] each (either may be NULL): the values
 * the ideal kernels evaluate (EXPLICIT: computed on the device by the same function) */
int adc_engine_bid_curves_fetch(adc_engine *e, double *impression_rate_host, double *cpc_host);
/* get_max_expected_bid_profits (experiment_metrics.py:40-61) for the CURRENT (drifted) parameters against the cached
 * curves: max expected profit and its argmax over the grid, per keyword; host outputs may be NULL.  With metrics
 * enabled the value is also added to the per-keyword ideal sums (raw, and with <= 0 replaced by 1 as compute_AKNCP
 * does, :71-75). */
/* diagnostic: per keyword, the grid points that can be the argmax of the expected profit for SOME margin sctr x rev_mean, each
 * with the margin interval on which it can (found once per adc_engine_bid_curves_build; adc_engine_ideal_step evaluates only
 * the few whose interval holds the day's margin): n_nk[N*K] (0xFFFF: the whole grid is evaluated), entries_nkc6[N*K][*cap][6]
 * = {interval lo, hi (float32 bits), curve point (2 words; EXPLICIT: 0, 0), grid index, 0}, ascending grid indices */
int adc_engine_bid_curves_contenders(adc_engine *e, uint16_t *n_nk, uint32_t *entries_nkc6, int32_t *cap);
int adc_engine_ideal_step(adc_engine *e, double *ideal_host_nk, int32_t *best_index_host_nk);
/* run_oracle_agent: next action := bid_grid[argmax] of the last adc_engine_ideal_step, budget as given */
int adc_engine_policy_oracle(adc_engine *e, float budget);

/* NaiveZeroMarginStrategy (adcraft/baselines/interpolated_expectations.py:442-515), one agent per env.
 * init: empty caches (:286-295), max_bids = 0.01 (:481), the agent's Philox stream keyed by seeds_n (NULL: derived
 * from adc_config.seed and the env id). */
int adc_engine_agent_init(adc_engine *e, float default_expected_revenue_per_conversion, const uint64_t *seeds_n);
/* update_all_caches (:485-494) with one observation per keyword: host arrays [N*K] (all three), or all NULL = the
 * engine's last observation where it lies on the device (after reset: zeros, as the reference's reset observation) */
int adc_engine_agent_update(adc_engine *e, const int32_t *clicks_nk, const int32_t *conversions_nk, const float *revenue_nk);
/* sample_action (:496-515) into the engine's action buffers (what adc_engine_step_device(e, NULL, NULL) consumes).
 * budget_override > 0 replaces the agent's 100 x sum(codes) budget (the notebooks pass budget = 100000 to the env).
 * replay_uniforms_nk (host double [N*K], nullable): the rng.random() value to use for each keyword instead of the
 * agent's Philox stream - parity mode against recorded reference runs. */
int adc_engine_agent_act(adc_engine *e, float budget_override, const double *replay_uniforms_nk);
/* update from the device-resident observation + act, one launch (the closed loop's per-step call) */
int adc_engine_agent_step(adc_engine *e, float budget_override);
/* caches to host (any pointer may be NULL): ave_rpc, num_rpc_obs, ave_sctr, num_sctr_obs, max_bids, each [N*K] */
int adc_engine_agent_state(adc_engine *e, float *ave_rpc_nk, int32_t *num_rpc_obs_nk, float *ave_sctr_nk,
                           int32_t *num_sctr_obs_nk, double *max_bids_nk);
/* NaiveInterpolationStrategy (adcraft/baselines/interpolated_expectations.py:298-439), one agent per env.  Its caches: the
 * rpc / sctr cache of the zero-margin agent, and per keyword two lists of interpolation points in cents 1..300 (keys outside
 * $0.01-$3.00 are only remembered through max_observed, the largest key seen): every observation creates or updates a
 * float32 mean of the clicks, an observation with clicks > 0 a float64 mean of cost / clicks.  Device memory: 24 bytes per
 * keyword and slot of capacity, plus 56 bytes per keyword.  The lists gain at most one point per update, so `capacity`
 * slots hold them while the updates since init number at most `capacity`; 0 = min(300, max_days + 1), at most 300 (which
 * never overflows).  An update that could overflow is refused with ADC_EINVAL before anything is enqueued; run_days checks
 * all of its days up front.
 * init: empty caches, own last bid 0.01 (the notebooks' first previous_action), the agent's Philox stream (stage 13) keyed by
 * seeds_n (NULL: derived from adc_config.seed and the env id).  threshold = profit_acquisition_threshold; allowed_bids: 1 to
 * 2048 finite values in any order.  Calling it again resets the agent; the capacity stays what the first call fixed. */
int adc_engine_interp_init(adc_engine *e, double profit_acquisition_threshold, double bid_step, const double *allowed_bids,
                           int32_t n_bids, int32_t capacity, const uint64_t *seeds_n);
/* agent.allowed_bids = bids (the notebooks grow the grid every day); same rules as at init */
int adc_engine_interp_set_allowed_bids(adc_engine *e, const double *bids, int32_t n);
/* update_all_caches (:400-403) with one observation per keyword: host arrays [N*K] (all five: the previous bids, finite, keyed
 * as float32; clicks, cost, conversions, revenue), or all NULL = the agent's own last bids and the engine's last observation
 * where it lies on the device */
int adc_engine_interp_update(adc_engine *e, const double *prev_bids_nk, const int32_t *clicks_nk, const float *cost_nk,
                             const int32_t *conversions_nk, const float *revenue_nk);
/* sample_action (:405-439) into the engine's action buffers: the bid as the env rounds it (to cents, >= 0.01), the budget as
 * the env rounds the agent's (cents, float32) or budget_override if > 0.  replay_uniforms_nk (host double [N*K], nullable):
 * the rng.random() value rng.choice uses for each keyword instead of the agent's stream (read only where a draw happens). */
int adc_engine_interp_act(adc_engine *e, float budget_override, const double *replay_uniforms_nk);
/* update from the device (own last bids, last observation) + act, one launch, no host sync (the closed loop's per-step call) */
int adc_engine_interp_step(adc_engine *e, float budget_override);
/* caches to host (any pointer may be NULL): [N*K] ave_rpc, num_rpc_obs, ave_sctr, num_sctr_obs, max_observed, the grid index
 * of the last act's bid (-1: no draw, bid 0.01); [N] the last act's float64 budget, profit_beliefs, cost_beliefs */
int adc_engine_interp_state(adc_engine *e, float *ave_rpc_nk, int32_t *num_rpc_obs_nk, float *ave_sctr_nk, int32_t *num_sctr_obs_nk,
                            double *max_observed_nk, int32_t *bid_index_nk, double *budget_n, double *profit_beliefs_n, double *cost_beliefs_n);
/* the interpolation points to host (any pointer may be NULL), slot-major [capacity][N*K], ascending cents in the first
 * n_*_nk slots: the clicks list (cent, ave_clicks, count) and the cpc list (cent, ave_cpc, count) */
int adc_engine_interp_entries(adc_engine *e, int32_t *capacity, int32_t *n_clicks_nk, uint16_t *clicks_cent_cnk, float *ave_clicks_cnk,
                              int32_t *clicks_count_cnk, int32_t *n_cpc_nk, uint16_t *cpc_cent_cnk, double *ave_cpc_cnk,
                              int32_t *cpc_count_cnk);
/* the engine's device action buffers to host (what a policy above, adc_engine_sample_actions or
 * adc_engine_set_flat_actions_device last wrote) */
int adc_engine_get_actions(adc_engine *e, float *bids_nk, float *budget_n);
/* `days` consecutive days of the device-resident loop in one call: per day, the policy writes the action
 * (FIXED_ACTIONS: whatever the action buffers hold; ZERO_MARGIN: adc_engine_agent_step, plus adc_engine_ideal_step when
 * curves are built; INTERPOLATION: the same with adc_engine_interp_step; ORACLE: adc_engine_ideal_step + adc_engine_policy_oracle), then the env steps.  Asynchronous on
 * the engine's stream.  adc_engine_day_graph_enable(e, 1) makes it replay pairs of days from a captured hipGraph
 * (same results; measured no faster on MI355X - the dependent kernels of a day are latency-, not launch-bound - and an engine
 * whose chain of days runs as env groups, see adc_engine_env_groups, keeps the plain chain, which is the faster of the two). */
enum adc_policy { ADC_POLICY_FIXED_ACTIONS = 0, ADC_POLICY_ZERO_MARGIN = 1, ADC_POLICY_ORACLE = 2, ADC_POLICY_INTERPOLATION = 3,
                  ADC_POLICY_MLP = 4 /* adc_engine_mlp_step per day, plus adc_engine_ideal_step when curves are built; never captured */ };
int adc_engine_run_days(adc_engine *e, int policy, int32_t days, float budget);
int adc_engine_day_graph_enable(adc_engine *e, int enabled);
/* per (env, keyword) metric sums to host (any pointer may be NULL): profit in cents, ideal, ideal with <= 0 -> 1;
 * per-env AKNCP = median_k(profit / ideal_pos), NCP = sum profit / sum ideal (experiment_metrics.py:64-83) */
int adc_engine_metrics_read_nk(adc_engine *e, int64_t *profit_cents_nk, double *ideal_sum_nk, double *ideal_pos_sum_nk);
/* the same two metrics reduced on the device: akncp_n[N] = median over the keywords of (profit / days) / (ideal_pos / days) (a
 * bitonic sort per env in LDS; numpy's median convention), ncp_n[N]; 2 N doubles cross the bus instead of 3 N K.
 * num_keywords <= 4096. */
int adc_engine_metrics_akncp_ncp(adc_engine *e, double days, double *akncp_n, double *ncp_n);

/* ---- the MLP policy: a learned agent on the device (parts/kernel_mlp_policy.inc; the law is csrc/adc_mlp.h) -----------
 * A fully connected policy network - and optionally a value network - of up to 4 Linear layers each, hidden widths up to 256,
 * tanh or relu between them, evaluated per env and day on the flat observation (the FlatArrayWrapper row, read from the
 * engine's output arrays; all zeros on the first day of an episode, also right after an auto-reset).  The policy network
 * ends in A = K + 1 means (flat action order [budget, bids...]) with a free log_std[A] vector, or in 2A values, means then
 * log-stds.  action = mean + exp(log_std) * z with z from the agent's own Philox stream (stage 14; the env's stream does
 * not move), or action = mean (deterministic), or z handed in (replay).  Bids go to the env as max(action, 0.01), clipped
 * above when bid_clip_hi > 0, rounded to cents; the budget as max(action[0], 0.01) or budget_override when that is > 0.
 * Every operation is a fixed sequence of correctly rounded float32 / float64 operations: adc_mlp_act_host gives the same
 * bits on the host. */
enum adc_mlp_activation { ADC_MLP_TANH = 0, ADC_MLP_RELU = 1 };
typedef struct adc_mlp_config {
    uint32_t struct_size;          /* sizeof(adc_mlp_config) */
    int32_t activation;            /* adc_mlp_activation */
    int32_t n_policy_layers;       /* 1..4 */
    int32_t policy_widths[4];      /* outputs of each policy layer; the last is A or 2A */
    int32_t n_value_layers;        /* 0 (no value network; values are 0) or 1..4 */
    int32_t value_widths[4];       /* outputs of each value layer; the last is 1 */
    int32_t normalize;             /* nonzero: x = (x - shift[j]) * scale[j] (adc_engine_mlp_set_norm) */
    int32_t clamp_log_std;         /* nonzero: log_std clamped to [log_std_lo, log_std_hi] */
    float log_std_lo, log_std_hi;
    float bid_clip_hi;             /* > 0: bids clipped above at this many dollars */
    int32_t deterministic;         /* nonzero: action = mean, no draws */
} adc_mlp_config;
/* shapes and options; every weight, bias and vector starts at zero and must be uploaded before the first act.  seeds_n (may be
 * NULL: keyed by the engine seed and the global env id) seeds the agents' streams, tick 0.  A second call re-initialises. */
int adc_engine_mlp_init(adc_engine *e, const adc_mlp_config *cfg, const uint64_t *seeds_n);
/* Observation history: adc_engine_mlp_init with a frame count `frames` = H in 1..8 (1: adc_engine_mlp_init itself, the same
 * kernels and bits).  With H > 1 the network input of an env is the concatenation of its last H flat observations,
 * D = H (5K + 2): x[f D0 + j], frame 0 today's row, frame f >= 1 the raw row that the act on episode day d - f read, or zeros
 * where the env has no such act in this episode (csrc/adc_mlp.h states the law: the per-env history hist[N][H][5K+2] of raw
 * frames, slot = episode day mod H, and the two validity words last / from).  The frames are gathered on the device.  Every
 * first layer has n_in = D; adc_engine_mlp_set_norm takes vectors of length D (normalisation is per position, zero frames
 * included); the rollout record's obs rows, the replay ring's rows, the running observation normalisers' vectors and the
 * trainers' shapes are D wide.  An auto-reset clears an env's history through its day 0; days stepped without the agent
 * restart it; adc_engine_reset forgets it for the envs it resets.  Not detected: an auto-reset followed by exactly last + 1
 * days without an act.  adc_engine_mlp_bootstrap_value and the trainers' stores read the row an act would read now and write
 * nothing.  Refused (ADC_EINVAL, the engine stays usable): frames outside 1..8; a stacked row that does not fit the act's LDS. */
int adc_engine_mlp_init_frames(adc_engine *e, const adc_mlp_config *cfg, const uint64_t *seeds_n, int32_t frames);
int adc_engine_mlp_frames(adc_engine *e, int32_t *frames);
/* the history to the host and back: hist_nhd [N][H][5K+2] raw frames, last_n / from_n [N] (any may be NULL); a run resumed from
 * them continues bit for bit.  ADC_ESTATE without a history (frames = 1). */
int adc_engine_mlp_history_get(adc_engine *e, float *hist_nhd, int32_t *last_n, int32_t *from_n);
int adc_engine_mlp_history_set(adc_engine *e, const float *hist_nhd, const int32_t *last_n, const int32_t *from_n);
/* Recurrent policy: adc_engine_mlp_init with one GRU cell of width gru_width = G in 1..256 in front of the policy network's output
 * layer (0: adc_engine_mlp_init itself, the same kernels and bits).  With n_policy_layers = L, layers 0 .. L-2 are the trunk as
 * ever, the cell reads the trunk's last activation (the input row when L = 1) and the env's state h[G], and the output layer L-1
 * has n_in = G and reads the new state; no activation follows the cell.  The cell is torch.nn.GRUCell's arithmetic, gates r, z, n
 * (csrc/adc_gru.h states the law, every operation one correctly rounded float32 / float64 operation; adc_gru_cell_host and
 * adc_mlp_act_recurrent_host give the same bits on the host).  Everything after the output layer - heads, sample, log-probability,
 * bids, budget - and the feed-forward value network on the input row are adc_engine_mlp_init's.
 * State: h[N][2][G] and two words per env, last and from, under the observation history's rule.  An act on episode day d starts
 * from zeros on day 0, after an auto-reset, after days stepped without the agent and after an explicit reset (adc_engine_reset
 * forgets the state of the envs it resets), else from the state the act of day d - 1 left; it writes the new state to slot d & 1,
 * so a second act on the same day (replayed normals) reads the same input state and writes the same bits.  Not detected, as for
 * the history: an auto-reset followed by exactly last + 1 days without an act.
 * adc_engine_mlp_act, _step, adc_engine_run_days(ADC_POLICY_MLP), the rollout record, adc_engine_mlp_last and
 * adc_engine_mlp_bootstrap_value work unchanged; adc_engine_mlp_set_layer(0, L-1, ...) is the output layer [G][P].
 * The flat parameter order (adc_engine_mlp_param_count, _get_params, _get_member_params, the evolution strategy) is: the trunk
 * layers, Wi input-major [n_in][3G], bi [3G], Wh [G][3G], bh [3G], the output layer.  adc_engine_mlp_population and adc_engine_es_*
 * work over it; adc_engine_es_perturb also forgets every env's state (it was computed under other weights).
 * Refused with ADC_EINVAL: gru_width outside 0..256; a cell whose state and gates do not fit the act's LDS.  Refused with ADC_ESTATE while the policy is recurrent, the engine staying usable:
 * adc_engine_mlp_set_squash, _set_bounds, adc_engine_mlp_learners, adc_engine_pg_*, td3_*, sac_*, im_*, adc_engine_teach_days and
 * adc_engine_dagger_days (training a recurrent policy is the evolution strategy's; an observation history, frames > 1, has no
 * recurrent init). */
int adc_engine_mlp_init_recurrent(adc_engine *e, const adc_mlp_config *cfg, const uint64_t *seeds_n, int32_t gru_width);
int adc_engine_mlp_gru_width(adc_engine *e, int32_t *width);       /* 0: feed-forward */
/* the cell, input-major as adc_engine_mlp_set_layer's weights: wi_in_3g [n_in][3G] (torch's weight_ih.T), bi_3g, wh_g_3g [G][3G]
 * (weight_hh.T), bh_3g; columns in gate order r | z | n.  ADC_ESTATE when the policy is not recurrent.  _member_: into one member
 * of a population. */
int adc_engine_mlp_set_gru(adc_engine *e, const float *wi_in_3g, const float *bi_3g, const float *wh_g_3g, const float *bh_3g);
int adc_engine_mlp_set_member_gru(adc_engine *e, int32_t member, const float *wi_in_3g, const float *bi_3g, const float *wh_g_3g,
                                  const float *bh_3g);
/* the state to the host and back: h_n2g [N][2][G], last_n / from_n [N] (any may be NULL); a run resumed from them continues bit
 * for bit.  forget: last = -2 for every env, whose next act starts from zeros.  ADC_ESTATE when the policy is not recurrent. */
int adc_engine_mlp_hidden_get(adc_engine *e, float *h_n2g, int32_t *last_n, int32_t *from_n);
int adc_engine_mlp_hidden_set(adc_engine *e, const float *h_n2g, const int32_t *last_n, const int32_t *from_n);
int adc_engine_mlp_hidden_forget(adc_engine *e);
/* one Linear layer: network 0 = policy, 1 = value; weights_in_out is [n_in][n_out] row-major (input-major: torch's
 * weight.T), bias [n_out].  May be called again at any time between days (a trainer's update); nothing else changes. */
int adc_engine_mlp_set_layer(adc_engine *e, int32_t network, int32_t layer, const float *weights_in_out, const float *bias_out);
int adc_engine_mlp_set_norm(adc_engine *e, const float *shift_d, const float *scale_d);
int adc_engine_mlp_set_log_std(adc_engine *e, const float *log_std_a);
int adc_engine_mlp_set_deterministic(adc_engine *e, int32_t deterministic);
/* the squashed action: with lo_a / hi_a [A] (finite, hi > lo) every later act gives the env e[a] = lo[a] + half[a] * (tanh(u[a]) + 1)
 * in place of the sampled action u[a] (half[a] = 0.5f * (hi[a] - lo[a]) formed once here; a sum, a product, a sum after the law's
 * tanh), and takes the bid and the budget from e as it took them from u; a deterministic act squashes the mean.  The record,
 * adc_engine_mlp_last, the log-probability and the ticks are untouched: they keep u.  Both NULL: off, and the act is bit for bit
 * what it was before the call.  adc_engine_mlp_init turns it off.  Refused with ADC_ESTATE while a population or learners are
 * active, and adc_engine_mlp_population / adc_engine_mlp_learners (members > 0) are refused with ADC_ESTATE while it is on. */
int adc_engine_mlp_set_squash(adc_engine *e, const float *lo_a, const float *hi_a);
/* the same squash for learners (adc_engine_mlp_learners, members > 0): one pair of bounds shared by all members; every member's
 * act gives its envs lo + half (tanh(u) + 1), and the record, adc_engine_mlp_last, the log-probability and the ticks keep u.
 * Accepted only while learners are active (ADC_ESTATE otherwise); both NULL: off.  It goes with the learners: dropped by
 * adc_engine_mlp_learners (any argument), by adc_engine_mlp_population (members > 0, which ends the learners) and by
 * adc_engine_mlp_init.  adc_engine_mlp_set_squash stays refused while learners are active, and adc_engine_mlp_learners /
 * adc_engine_mlp_population (members > 0) stay refused while the single policy's squash is on: this is the learners' own entry
 * point. */
int adc_engine_mlp_learners_set_squash(adc_engine *e, const float *lo_a, const float *hi_a);
/* the bounded act (csrc/adc_mlp.h "bounded"): the deterministic actor squashed into the action box, as RLlib's DDPG family and
 * Stable-Baselines3 run TD3.  With lo_a / hi_a [K + 1] (flat action order: budget, bids; finite, hi > lo) the action is
 * n = clamp(tanh(mean) + exp(log_std) z, -1, 1) in units of the box - n = tanh(mean) for a deterministic act - the env is given
 * e = lo + 0.5 (hi - lo) (n + 1), and the record, adc_engine_mlp_last's action and a trainer's ring hold n; mean stays the raw
 * mean, the log-probability is +0, the ticks move as ever.  exp(log_std) is so in units of the half-range.  A deterministic
 * bounded act gives the env the bits adc_engine_mlp_set_squash plus a deterministic act give it.  Both NULL: off (the exploration
 * mode is back to gaussian), and the act is bit for bit what it was before the call; adc_engine_mlp_init turns it off.
 * Refused with ADC_ESTATE: together with adc_engine_mlp_set_squash (either order), with a two-headed policy, while a population
 * is active (adc_engine_mlp_population, and so the evolution strategy, is refused while it is on), while learners are active
 * (theirs is adc_engine_mlp_learners_set_bounds: one pair shared by all members, accepted only while learners are active, gone
 * with them), and while a TD3 ring holds transitions (their actions are in units of the bounds as they are).  While it is on,
 * adc_engine_pg_*, adc_engine_im_* and adc_engine_sac_* are refused (they need a log-probability), and adc_engine_teach_days
 * records the teacher's action e as n = clamp((e - lo) / half - 1, -1, 1) (the division as a product with 1 / half). */
int adc_engine_mlp_set_bounds(adc_engine *e, const float *lo_a, const float *hi_a);
int adc_engine_mlp_learners_set_bounds(adc_engine *e, const float *lo_a, const float *hi_a);
/* the bounded act's exploration: ADC_MLP_EXPLORE_GAUSSIAN (the default) or ADC_MLP_EXPLORE_RANDOM, the warm-up: n uniform in
 * (-1, 1) from the very word the normal would have been made from (handed-in normals are not read; the ticks move as ever; a
 * deterministic act stays tanh(mean)).  ADC_MLP_EXPLORE_RANDOM needs the bounds (ADC_ESTATE otherwise). */
enum adc_mlp_explore { ADC_MLP_EXPLORE_GAUSSIAN = 0, ADC_MLP_EXPLORE_RANDOM = 1 };
int adc_engine_mlp_set_explore(adc_engine *e, int32_t mode);
/* what the two calls above left: lo_a / hi_a [K + 1] (written only while the bounds are on; either may be NULL), *bounded 0 / 1,
 * *explore - what a checkpoint has to carry */
int adc_engine_mlp_get_bounds(adc_engine *e, float *lo_a, float *hi_a, int32_t *bounded, int32_t *explore);
/* host twins (adc_shims.cpp), the code the device runs.  adc_mlp_bounded_host: the bounded act's head on `count` components from
 * their raw means and log-stds: mode 0 explore (gaussian; normals_a, or NULL: drawn from agent_key / tick), 1 deterministic,
 * 2 explore (random); n_a the action, env_a its box image (either may be NULL).  adc_mlp_unbox_host: a teacher's actions e_a to n_a */
int adc_mlp_bounded_host(int32_t count, const float *mean_a, const float *log_std_a, const float *normals_a, uint64_t agent_key, uint32_t tick,
                         int32_t mode, const float *lo_a, const float *hi_a, float *n_a, float *env_a);
int adc_mlp_unbox_host(int32_t count, const float *e_a, const float *lo_a, const float *hi_a, float *n_a);
/* act on the observation the last step left: actions into the engine's action buffers; replay_normals_na (may be NULL)
 * replaces the draws.  Every act moves the agents' ticks on by one.  Not recorded. */
int adc_engine_mlp_act(adc_engine *e, float budget_override, const float *replay_normals_na);
/* act + the env's step on the device (chain-compatible, like adc_engine_step_device); recorded when a rollout record is on */
int adc_engine_mlp_step(adc_engine *e, float budget_override);
/* the last act's means, clamped log-stds, unclipped actions [N][A], log-probabilities and values [N] (any may be NULL) */
int adc_engine_mlp_last(adc_engine *e, float *mean_na, float *log_std_na, float *action_na, float *logp_n, float *value_n);
/* the value network on the observation the last step left (zeros for an env that has just been reset): the bootstrap value */
int adc_engine_mlp_bootstrap_value(adc_engine *e, float *value_n);
/* the agents' own streams: key and tick [N] of every env's agent (either may be NULL); every act moves a tick on by one */
int adc_engine_mlp_agent_state(adc_engine *e, uint64_t *keys_n, uint32_t *ticks_n);
/* the rollout record: per recorded day t < horizon and env the unclipped action [A], log-probability, value, reward (float32
 * of the step's float64 reward), terminated, truncated and - with ADC_ROLLOUT_OBS - the network's input [D]; arrays laid out
 * [T][N][...], on the device (ADC_BUF_ROLLOUT_*) and fetched to the host.  adc_engine_mlp_step and adc_engine_run_days
 * (ADC_POLICY_MLP) record; a day past the horizon is refused until adc_engine_rollout_reset.  horizon 0 turns it off. */
enum adc_rollout_fields { ADC_ROLLOUT_OBS = 1 };
int adc_engine_rollout_enable(adc_engine *e, int32_t horizon, int32_t fields);
int adc_engine_rollout_reset(adc_engine *e);
/* *days_recorded and the first that many days of every array asked for (any pointer may be NULL) */
int adc_engine_rollout_fetch(adc_engine *e, int32_t *days_recorded, float *action_tna, float *logp_tn, float *value_tn, float *reward_tn,
                             uint8_t *terminated_tn, uint8_t *truncated_tn, float *obs_tnd);

/* ---- policy populations: per-member weights of the policy network (parts/kernel_es.inc) ------------------------------------
 * After adc_engine_mlp_init, `members` = M > 0 gives the engine M copies of the POLICY network's layers (weights and biases),
 * each starting as the centre policy (what adc_engine_mlp_set_layer uploaded), and every env the member it evaluates:
 * member_of_env_n[N] with entries in [0, M), or NULL for env / (N / M) (M must then divide N).  The value network, log_std,
 * the normalisation vectors and the clamps stay shared by all members.  M = 0 turns the population off (the default: every
 * env runs the centre).  Acts, steps, the rollout record, adc_engine_mlp_last and adc_engine_mlp_bootstrap_value work
 * unchanged.  A population does not survive adc_engine_mlp_init, and a new population drops the evolution strategy over the
 * old one.  adc_engine_mlp_set_layer keeps writing the centre alone.
 * The flat parameter order (length P, adc_engine_mlp_param_count): the policy layers in order, each W[j][h] input-major
 * (index j * n_out + h) followed by its b[h]. */
int adc_engine_mlp_population(adc_engine *e, int32_t members, const int32_t *member_of_env_n);
int adc_engine_mlp_set_member_layer(adc_engine *e, int32_t member, int32_t layer, const float *weights_in_out, const float *bias_out);
int adc_engine_mlp_param_count(adc_engine *e, int64_t *count);
int adc_engine_mlp_get_params(adc_engine *e, float *flat_p);                              /* the centre */
int adc_engine_mlp_get_member_params(adc_engine *e, int32_t member, float *flat_p);

/* ---- learners: per-member policy layers, value layers and log_std (the members of adc_engine_pg_pop_*) -------------------------
 * A second kind of population, for learners that train: `members` = M > 0 (M must divide num_envs, at most 65535) gives every
 * member its own policy layers, value layers and - with the free head - log_std[A], each starting as the centre (what
 * adc_engine_mlp_set_layer / _set_log_std uploaded); env -> member is env / (N / M), so member m owns the envs
 * [m N / M, (m + 1) N / M).  The normalisation vectors, the clamps, the activation and the shapes stay shared.  M = 0 turns the
 * mode off.  Acts, adc_engine_mlp_step, adc_engine_run_days(ADC_POLICY_MLP), the rollout record, adc_engine_mlp_last and
 * adc_engine_mlp_bootstrap_value work unchanged, every env under its member's networks: what member m's envs compute is, bit
 * for bit, what an engine of N / M envs at env_id_base + m N / M computes under that member's weights.  This mode and
 * adc_engine_mlp_population exclude each other: starting one drops the other with the strategy or trainer over it;
 * adc_engine_mlp_init drops both.  adc_engine_mlp_set_layer and adc_engine_mlp_set_log_std keep writing the centre alone.
 * adc_engine_mlp_get_learner_params: the member's parameters in the trainer's flat order theta[Q] (adc_pg_param_count_host): the
 * policy layers, the value layers, then log_std. */
int adc_engine_mlp_learners(adc_engine *e, int32_t members);
/* network: 0 policy, 1 value; weights [n_in][n_out] input-major as adc_engine_mlp_set_layer's */
int adc_engine_mlp_set_learner_layer(adc_engine *e, int32_t member, int32_t network, int32_t layer, const float *weights_in_out, const float *bias_out);
int adc_engine_mlp_set_learner_log_std(adc_engine *e, int32_t member, const float *log_std_a);
int adc_engine_mlp_get_learner_params(adc_engine *e, int32_t member, float *theta_q);

/* ---- an evolution strategy on the device (OpenAI-ES; the law is csrc/adc_es.h) ----------------------------------------------
 * Over a population of an even number of members: adc_engine_es_perturb writes member 2i / 2i + 1 = theta +- sigma * eps(i, g)
 * from counter-addressed noise (Philox stage 15 under the strategy's own key; never stored), zeroes every env's return and
 * turns accumulation on: every day stepped by adc_engine_mlp_step / adc_engine_run_days(ADC_POLICY_MLP) adds the env's float64
 * reward to its return (through auto-resets too: fitness is the reward summed over the generation's days).  A member's fitness
 * is the float64 mean of its envs' returns.  adc_engine_es_update shapes the fitness (the device's, or fitness_m[M] handed in),
 * forms the gradient estimate with the noise regenerated, takes an Adam or SGD ascent step on theta, rebuilds the centre policy
 * from it (so evaluation without a population and adc_engine_mlp_get_params see the new theta), moves the generation on by one
 * and turns accumulation off.  theta starts as the centre policy at adc_engine_es_init; later adc_engine_mlp_set_layer calls do
 * not reach it (adc_engine_es_state_set does). */
enum adc_es_shaping { ADC_ES_CENTERED_RANK = 0, ADC_ES_RAW = 1 };
enum adc_es_optimiser { ADC_ES_ADAM = 0, ADC_ES_SGD = 1 };
typedef struct adc_es_config {
    uint32_t struct_size;          /* sizeof(adc_es_config) */
    float sigma;                   /* > 0: the perturbation's standard deviation */
    float lr;                      /* >= 0 */
    float beta1, beta2, eps;       /* Adam: 0 <= beta < 1, eps > 0 */
    float l2;                      /* >= 0: gradient g - l2 * theta */
    int32_t shaping;               /* adc_es_shaping */
    int32_t optimiser;             /* adc_es_optimiser */
    uint64_t seed;                 /* the noise's seed; 0: the engine's seed */
} adc_es_config;
typedef struct adc_es_stats {
    int64_t generation;            /* after the update */
    double fitness_mean, fitness_max, fitness_min;
    double grad_norm, theta_norm;  /* Euclidean norms of the (decayed) gradient estimate and of the new theta */
} adc_es_stats;
int adc_engine_es_init(adc_engine *e, const adc_es_config *cfg);
int adc_engine_es_perturb(adc_engine *e);
int adc_engine_es_fitness(adc_engine *e, double *fitness_m);
/* fitness_m may be NULL (the device's fitness: at least one day must have been stepped since the perturbation); stats may be NULL */
int adc_engine_es_update(adc_engine *e, const double *fitness_m, adc_es_stats *stats);
/* theta, the Adam moments [P] and the generation: a run resumed from them continues bit for bit (get: any pointer may be NULL) */
int adc_engine_es_state_get(adc_engine *e, float *theta_p, float *m_p, float *v_p, int64_t *generation);
int adc_engine_es_state_set(adc_engine *e, const float *theta_p, const float *m_p, const float *v_p, int64_t generation);

/* ---- policy-gradient training on the device: GAE, the networks' backward pass, PPO-clip / A2C (the law is csrc/adc_pg.h) --------
 * The consumer of the rollout record: with a record enabled with ADC_ROLLOUT_OBS and days recorded by adc_engine_mlp_step /
 * adc_engine_run_days(ADC_POLICY_MLP) under a stochastic policy, adc_engine_pg_advantages computes returns and advantages from
 * the record and the bootstrap value, adc_engine_pg_minibatch takes one gradient of the PPO-clip loss over every recorded day of
 * an env range and one Adam / SGD step, and writes the new parameters into the device's policy layers, value layers and log_std
 * (adc_engine_mlp_act, the next recorded day and adc_engine_mlp_get_params see them at once).  Nothing of the record leaves the
 * device.  Training takes no random draws: the envs' and agents' streams do not move.  The flat parameter order theta[Q]
 * (adc_engine_pg_param_count): the policy layers as in adc_engine_mlp_get_params, then the value layers in the same form, then
 * log_std[A] when the head is the free vector.  theta starts as the device's weights at adc_engine_pg_init; later
 * adc_engine_mlp_set_layer calls do not reach it (adc_engine_pg_state_set does).  Refused (ADC_ESTATE / ADC_EINVAL, the engine
 * stays usable): before adc_engine_mlp_init and its uploads, without a record or without ADC_ROLLOUT_OBS, with no day recorded,
 * with a population active, with a record that holds days collected deterministically. */
enum adc_pg_optimiser { ADC_PG_ADAM = 0, ADC_PG_SGD = 1 };
typedef struct adc_pg_config {
    uint32_t struct_size;          /* sizeof(adc_pg_config) */
    float gamma, lambda;           /* in [0, 1] */
    float eps_clip;                /* PPO's clip range; <= 0: no clip (the vanilla policy gradient; one epoch of it is A2C) */
    float vf_coef, ent_coef;       /* >= 0 */
    float reward_scale;            /* finite, != 0: rewards are multiplied by it before GAE */
    int32_t normalize_advantages;  /* over all recorded samples */
    float max_grad_norm;           /* > 0: clip the gradient's global norm; 0: off */
    int32_t optimiser;             /* adc_pg_optimiser */
    float lr;                      /* >= 0 */
    float beta1, beta2, eps;       /* Adam: 0 <= beta < 1, eps > 0 */
    int32_t minibatch_envs;        /* envs of a minibatch (whole trajectories); must divide num_envs; 0: all */
} adc_pg_config;
typedef struct adc_pg_stats {
    int64_t steps;                 /* optimiser steps taken so far */
    int64_t samples;               /* samples of the (last) minibatch */
    double policy_loss, value_loss, entropy, approx_kl, clip_fraction;
    double grad_norm;              /* before the clip */
    double explained_variance;     /* of the value function at collection, over the minibatch */
} adc_pg_stats;
int adc_engine_pg_init(adc_engine *e, const adc_pg_config *cfg);
int adc_engine_pg_param_count(adc_engine *e, int64_t *count);
/* returns and advantages of the recorded days (the bootstrap value is evaluated here); fetch: [T][N] each, either may be NULL */
int adc_engine_pg_advantages(adc_engine *e);
int adc_engine_pg_advantages_fetch(adc_engine *e, float *adv_tn, float *ret_tn);
/* one gradient and one optimiser step over every recorded day of the envs [env_begin, env_begin + env_count), env_count at most
 * the configuration's minibatch_envs; needs adc_engine_pg_advantages since the last recorded day.  stats may be NULL */
int adc_engine_pg_minibatch(adc_engine *e, int32_t env_begin, int32_t env_count, adc_pg_stats *stats);
/* advantages once, then `epochs` times the minibatches in ascending env order; stats (may be NULL): the last epoch's, averaged over
 * its minibatches in order (steps: the total so far) */
int adc_engine_pg_update(adc_engine *e, int32_t epochs, adc_pg_stats *stats);
/* theta, the Adam moments [Q] and the step count: a run resumed from them continues bit for bit (get: any pointer may be NULL) */
int adc_engine_pg_state_get(adc_engine *e, float *theta_q, float *m_q, float *v_q, int64_t *steps);
int adc_engine_pg_state_set(adc_engine *e, const float *theta_q, const float *m_q, const float *v_q, int64_t steps);

/* ---- learner populations: M independent PPO / A2C learners in lock-step on one engine -------------------------------------------
 * Over learners (adc_engine_mlp_learners): member m trains its own networks on the recorded days of its own envs
 * [m n, (m + 1) n), n = N / M, under its own adc_pg_config, and every kernel launch of an update covers all members: the
 * launches and host round trips of an update do not grow with M.  The law is csrc/adc_pg.h as it is: everything member m
 * computes - advantages, returns, gradient, theta / m / v after every step, statistics - is bit for bit what adc_engine_pg_*
 * computes on an engine of n envs at env_id_base + m n with the same parameter planes, agent seeds, initial weights and
 * configuration.  Sample s of the member's minibatch i is day s / mb, env m n + i mb + s % mb; the chunked sums run over the
 * member's own samples in that order, the advantage normalisation over its T n samples at index t n + local env.
 * adc_pg_pop_config_check (host only): every configuration passes adc_pg_config_check; count is 1 (shared) or `members`;
 * minibatch_envs is equal in all and divides num_envs / members (0: all of a member's envs); every other field may differ per
 * member.  adc_engine_pg_pop_init needs learners, a record with ADC_ROLLOUT_OBS and no other trainer alive (adc_engine_pg_init
 * and adc_engine_td3_init in turn refuse while learners are active); every member's theta starts as its device weights; a
 * refused allocation is ADC_ENOMEM and leaves the engine as it was.  The trainer does not survive adc_engine_mlp_init,
 * adc_engine_mlp_learners or adc_engine_rollout_enable. */
int adc_pg_pop_config_check(const adc_pg_config *cfgs, int32_t count, int32_t num_envs, int32_t members, const char **message);
int adc_engine_pg_pop_init(adc_engine *e, const adc_pg_config *cfgs, int32_t count);
/* GAE with the env's member's gamma, lambda and reward_scale; the normalisation per member that asks for it */
int adc_engine_pg_pop_advantages(adc_engine *e);
int adc_engine_pg_pop_advantages_fetch(adc_engine *e, float *adv_tn, float *ret_tn);       /* [T][N] each, either may be NULL */
/* minibatch `index` (0 .. n / minibatch_envs - 1) of every member: one gradient and one optimiser step each; stats_m[M] or NULL */
int adc_engine_pg_pop_minibatch(adc_engine *e, int32_t index, adc_pg_stats *stats_m);
/* advantages once, then `epochs` times the minibatches ascending; stats_m[M] (may be NULL) filled as adc_engine_pg_update fills its one */
int adc_engine_pg_pop_update(adc_engine *e, int32_t epochs, adc_pg_stats *stats_m);
/* one member's theta, Adam moments [Q] and step count (get: any pointer may be NULL); set also rebuilds the member's layers */
int adc_engine_pg_pop_state_get(adc_engine *e, int32_t member, float *theta_q, float *m_q, float *v_q, int64_t *steps);
int adc_engine_pg_pop_state_set(adc_engine *e, int32_t member, const float *theta_q, const float *m_q, const float *v_q, int64_t steps);
/* a member's hyperparameters from the next call on (minibatch_envs may not change); advantages must be computed again */
int adc_engine_pg_pop_set_config(adc_engine *e, int32_t member, const adc_pg_config *cfg);
/* theta, moments and step count of src into dst on the device, and dst's layers and log_std rebuilt (its configuration stays) */
int adc_engine_pg_pop_copy(adc_engine *e, int32_t src, int32_t dst);

/* ---- PPO with an adaptive KL penalty and a value-loss clip (the law is csrc/adc_pg_kl.h) ----------------------------------------
 * An add-on to a live PPO / A2C trainer (adc_engine_pg_init or adc_engine_pg_pop_init), attached after it as the reward
 * normaliser is: the loss gains kl_coef * mean KL(pi_old || pi_new), the analytic KL divergence between the diagonal Gaussian that
 * collected a sample and the current one, and a sample whose squared value error exceeds vf_clip has the value loss 0.5 vf_clip
 * and passes no gradient to the value network - RLlib's PPO loss (our value loss carries a factor 0.5 RLlib's does not: its
 * vf_loss_coeff 1.0 with vf_clip_param c is vf_coef 2.0 with vf_clip c here).  adc_pg_config, adc_pg_stats and every existing
 * entry point keep their layout and meaning; without adc_engine_pg_kl_init every call launches the kernels it launched.
 * The old distribution is a snapshot: while the add-on lives adc_engine_pg_advantages / _pg_pop_advantages (and so _pg_update /
 * _pg_pop_update, once at their start) also run the policy network alone over all recorded rows under the parameters then in
 * force and keep mean_old [T][N][A] and ls_old ([T][N][A] with two heads; with the free head the clamped log_std vector [A], one
 * per member under a population [M][A]) - bit for bit what the act computed.  adc_engine_pg_kl_old_dist_fetch copies them out.
 * The coefficient is the add-on's whole state.  adc_engine_pg_update / _pg_pop_update adapt it once at their end when
 * `adaptive`: kl, the float64 mean KL of the last epoch (the mean over its minibatches, as adc_pg_stats is), above 2 kl_target:
 * coef *= factor_up; below 0.5 kl_target: coef *= factor_down.  adc_engine_pg_minibatch / _pg_pop_minibatch never adapt: a
 * caller that drives minibatches itself uses _coef_set.  kl_coef == 0 adds nothing to the gradient (the trainer's own bits) and
 * still measures the KL.  Under a population every member has its own coefficient that adapts on its own, also when the settings
 * are shared (count 1); the adaptation of all members is one small upload, adc_engine_pg_pop_copy and a PBT round's copy give
 * the destination its donor's coefficient (it is not a tuned PBT hyperparameter).  With adc_engine_pg_state_get / _set (or the
 * _pg_pop_ ones) and _coef_get / _coef_set a resumed run continues bit for bit.
 * adc_engine_pg_kl_init is refused with ADC_ESTATE (the engine stays usable) without a live PPO / A2C trainer or while a TD3
 * trainer lives, with ADC_EINVAL when count is neither 1 nor the number of members (1 for adc_engine_pg_init) or a configuration
 * fails adc_pg_kl_config_check; it marks the advantages stale (a minibatch needs the snapshot).  The add-on does not survive
 * adc_engine_pg_init, adc_engine_pg_pop_init, adc_engine_mlp_init, adc_engine_mlp_learners or adc_engine_rollout_enable.
 * adc_engine_pg_kl_stats: of the last minibatch or update, [1] or [M]: kl and vf_clip_fraction as adc_pg_stats' fields are
 * formed, kl_coef the coefficient the gradient used, kl_coef_next the one the next call uses. */
typedef struct adc_pg_kl_config {
    uint32_t struct_size;          /* sizeof(adc_pg_kl_config) */
    float kl_coef;                 /* >= 0, finite: the starting coefficient */
    float kl_target;               /* > 0 and finite when adaptive */
    int32_t adaptive;              /* 0: the coefficient stays */
    float factor_up, factor_down;  /* > 1 and finite; in (0, 1); 0 means 1.5 / 0.5 */
    float vf_clip;                 /* >= 0, finite: the cap of a sample's squared value error; 0: off */
} adc_pg_kl_config;
typedef struct adc_pg_kl_stats {
    double kl, vf_clip_fraction;
    float kl_coef, kl_coef_next;
} adc_pg_kl_stats;
int adc_pg_kl_config_check(const adc_pg_kl_config *cfg, const char **message);           /* host only */
int adc_engine_pg_kl_init(adc_engine *e, const adc_pg_kl_config *cfgs, int32_t count);
int adc_engine_pg_kl_stats(adc_engine *e, adc_pg_kl_stats *stats_m);
int adc_engine_pg_kl_coef_get(adc_engine *e, int32_t member, float *coef);
int adc_engine_pg_kl_coef_set(adc_engine *e, int32_t member, float coef);
/* the snapshot of the last advantages call: mean_old_tna [T][N][A]; ls_old [T][N][A] (two heads) or [members][A] (either may be NULL) */
int adc_engine_pg_kl_old_dist_fetch(adc_engine *e, float *mean_old_tna, float *ls_old);

/* ---- PPO with shuffled sample-level minibatches and target-KL early stopping (the law is csrc/adc_pg_shuffle.h) ----------------
 * An add-on to a live PPO / A2C trainer (adc_engine_pg_init or adc_engine_pg_pop_init), attached after it in either order with
 * the KL add-on and the normalisers.  Without it a minibatch is every recorded day of a contiguous env range; with it a member's
 * n_s = T * n recorded samples (n its envs) are visited in a new pseudo-random order every epoch and a minibatch is
 * minibatch_samples consecutive positions of that order - RLlib's sgd_minibatch_size, Stable-Baselines3's batch_size - the last
 * of an epoch possibly short.  The order is a counter-addressed permutation (a 4-round Feistel network over the engine's Philox
 * stream with cycle walking): no sort, no state; its tick is the low 32 bits of the member's optimiser step count when the order
 * is drawn, so adc_engine_pg_state_get / _set (and the _pg_pop_ ones) carry all a bit-for-bit resume needs, and
 * adc_engine_pg_pop_copy and a PBT round need nothing new.  adc_pg_config, adc_pg_stats, adc_pg_kl_* and every existing entry
 * point keep their layout and meaning; without adc_engine_pg_shuffle_init every call launches the kernels it launched, and while
 * the add-on lives adc_engine_pg_minibatch / _pg_pop_minibatch over env ranges keep working.
 * While the add-on lives adc_engine_pg_update / _pg_pop_update run: the advantages once (and the KL add-on's snapshot), then per
 * epoch a new order and its ceil(n_s / minibatch_samples) minibatches.  target_kl > 0: a minibatch whose approx_kl (adc_pg_stats)
 * exceeds 1.5 target_kl ends the member's update BEFORE its optimiser step - the step count does not advance; under a population
 * the other members go on in the same launches and the stopped member's parameters and moments stay bit for bit.  The statistics
 * of an update are the means over the evaluated minibatches of the last epoch the member began, the stopping one included (so is
 * what the KL add-on adapts on); adc_pg_stats.samples is the last evaluated minibatch's count.
 * A caller may drive the minibatches itself: adc_engine_pg_advantages / _pg_pop_advantages (begins an update: no member has
 * stopped, no order is drawn), adc_engine_pg_shuffle_epoch (a new order for every member), adc_engine_pg_shuffle_minibatch(index)
 * in any order of indices; a member that has stopped is left as it is until the next advantages, and its adc_pg_stats of a later
 * minibatch are zero but for steps and samples (solo nothing is launched for it; under a population the launches cover it).
 * adc_engine_pg_shuffle_init makes sure the scratch holds max(horizon x minibatch_envs, minibatch_samples) samples per member
 * (allocated before the old arrays go: a refused allocation leaves the engine as it was).  It is refused with ADC_ESTATE (the
 * engine stays usable) without a live PPO / A2C trainer or while a TD3 trainer lives, with ADC_EINVAL when count is neither 1 nor
 * the number of members, the members' minibatch_samples differ, minibatch_samples exceeds horizon x envs of a member, or a
 * configuration fails adc_pg_shuffle_config_check.  adc_engine_pg_shuffle_minibatch is refused with ADC_ESTATE before the
 * advantages or before adc_engine_pg_shuffle_epoch since them, with ADC_EINVAL for an index outside the epoch.  The add-on does
 * not survive what the KL add-on does not survive. */
typedef struct adc_pg_shuffle_config {
    uint32_t struct_size;          /* sizeof(adc_pg_shuffle_config) */
    int32_t minibatch_samples;     /* >= 1; equal in all members; at most horizon x envs of a member */
    uint64_t seed;                 /* 0: the engine's */
    float target_kl;               /* >= 0, finite; 0: never stop */
} adc_pg_shuffle_config;
typedef struct adc_pg_shuffle_stats {
    int32_t epochs_begun, minibatches_evaluated, steps_taken, stopped;      /* of the last update */
} adc_pg_shuffle_stats;
int adc_pg_shuffle_config_check(const adc_pg_shuffle_config *cfg, const char **message);      /* host only */
int adc_engine_pg_shuffle_init(adc_engine *e, const adc_pg_shuffle_config *cfgs, int32_t count);      /* count 1 or members */
int adc_engine_pg_shuffle_epoch(adc_engine *e);                /* draw the order of a new epoch for every member */
int adc_engine_pg_shuffle_minibatch(adc_engine *e, int32_t index, adc_pg_stats *stats_m);     /* [1] or [M]; honours target_kl */
/* the order last drawn: the sample indices and their record rows, [members][n_s] each (either may be NULL), n_s of the days recorded;
 * ADC_ESTATE once the advantages are stale (a day recorded, adc_engine_rollout_reset, a changed configuration) or before an order */
int adc_engine_pg_shuffle_order_fetch(adc_engine *e, uint32_t *order, uint32_t *rows);
int adc_engine_pg_shuffle_stats(adc_engine *e, adc_pg_shuffle_stats *stats_m);         /* [1] or [M] */

/* ---- the queued update: adc_engine_pg_update / _pg_pop_update enqueued as one chain, one host wait ------------------------------
 * The same arguments, the same results: the learner state (adc_engine_pg_state_get / _pg_pop_state_get, the device's layers), the
 * returned statistics, adc_engine_pg_shuffle_stats, adc_engine_pg_kl_stats and the adapted KL coefficients are bit for bit those
 * of the host-driven call, with or without either add-on, the normalisers or a PBT scheduler; the two may be mixed freely from one
 * update to the next.  The host-driven update waits for every minibatch's sums to decide two things before the step - whether
 * the target-KL stop fires, and the norm clip's scale; here a one-wave kernel decides them on the device by the same law
 * (adc_pg_decide_host is its host twin), every other kernel of the chain passes a stopped member by, and the host waits once, for
 * the log of the minibatches' raw sums, from which it finishes the statistics as the host-driven loops do.  After the advantages
 * (whose moment fetches are as they were) the call uploads its tables once - the step constants of the steps
 * s0 ... s0 + epochs x minibatches - 1, every epoch's shuffle tick (a member that has not stopped has taken exactly
 * s0 + epoch x minibatches steps when an epoch begins), a population's member table - and enqueues epochs x minibatches
 * minibatches whatever stops: a stopped member's launches run and return at once.  The log, the control blocks and the tables are
 * allocated at the first call and grown on demand (ADC_ENOMEM leaves the engine as it was); epochs x minibatches is at most 2^22.
 * Under shuffled minibatches no order survives the call: adc_engine_pg_shuffle_minibatch / _order_fetch are refused with
 * ADC_ESTATE until adc_engine_pg_shuffle_epoch draws one.  Otherwise refused as adc_engine_pg_update / _pg_pop_update are. */
int adc_engine_pg_update_queued(adc_engine *e, int32_t epochs, adc_pg_stats *stats);
int adc_engine_pg_pop_update_queued(adc_engine *e, int32_t epochs, adc_pg_stats *stats_m);

/* ---- imitation learning on the device: teacher days, behaviour cloning and MARWIL (the law is csrc/adc_imitation.h) -------------
 * A TEACHER DAY is an act of the learned agent whose action is thrown away and replaced by an expert's.  Per day, chained and
 * group-compatible like a day of adc_engine_run_days(ADC_POLICY_MLP): the learner acts on the observation the last step left as
 * adc_engine_mlp_step has it act - static normalisation, observation history, value network, its tick moves on by one - but its
 * bids and budget go to a scratch buffer; the record's slot gets the network input row and the value.  Then the teacher acts as
 * adc_engine_run_days has it act for that policy (ADC_POLICY_FIXED_ACTIONS: the action buffers as they are - how labels of any
 * outside expert get in), the slot's action becomes {budget, bids} the step is about to consume (float32) and its logp +0, and the
 * env steps.  The env ends a teacher day in exactly the state adc_engine_run_days(teacher) leaves it in.
 * The engine counts the record's teacher days (cleared by adc_engine_rollout_enable / _reset).  The policy-gradient calls refuse a
 * record that holds any ("the record holds teacher days"), adc_engine_td3_store accepts them (demonstrations), the SAC stores
 * refuse them (the ring would need the pre-squash action).  adc_engine_teach_days is refused (ADC_ESTATE / ADC_EINVAL, the engine
 * stays usable): ADC_POLICY_MLP as the teacher, before adc_engine_mlp_init and its uploads, without a record or without
 * ADC_ROLLOUT_OBS, without room for `days`, with a population or learners active, with a squash set, with a teacher that has not
 * been initialised (adc_engine_run_days' messages). */
int adc_engine_teach_days(adc_engine *e, int teacher_policy, int32_t days, float budget);

/* A DAGGER DAY (Ross, Gordon and Bagnell 2011; the law is csrc/adc_dagger.h) is a teacher day on which a per-env coin picks whose
 * action the step consumes.  Both agents act on the same observation exactly as on a teacher day - the learner into the scratch,
 * the teacher into the engine's action buffers - then one kernel writes the record's action (the teacher's {budget, bids}: the
 * LABEL, in units of the box under the bounded act; logp +0), copies the teacher's action over the learner's in the scratch for
 * the envs whose coin picks the teacher, and notes the coin in a mask; the step consumes the scratch.  The engine's action buffers
 * are left holding the teacher's action: a ADC_POLICY_FIXED_ACTIONS teacher keeps labelling day after day, and
 * adc_engine_get_actions after a DAgger day returns the label.  The coin of env e is word x of draw(agent key of e, 0, stage 23,
 * 0, the agent's tick before the day's act) against round(beta * 2^32): beta = 1 is a teacher day bit for bit, beta = 0 the
 * learner's own day with the teacher's label.  It adds no state and moves no other stream.
 * A DAgger day counts as a teacher day (the policy-gradient calls and the SAC stores refuse the record, adc_engine_im_* accept it)
 * and in a count of its own, cleared with the teacher days': adc_engine_td3_store refuses a record that holds one (the recorded
 * action is not the one the step consumed), and so do adc_engine_im_advantages / _im_minibatch / _im_update under beta != 0
 * (MARWIL's weight needs returns that follow the labelled action; the value loss under vf_coef stays allowed and fits the value
 * network to the mixture's returns).  Dataset aggregation is the record itself: enable it with T = rounds x days and do not reset
 * it between rounds - adc_engine_im_advantages / _im_update run over all days recorded so far.
 * Refused as adc_engine_teach_days is, and: beta outside [0, 1] or NaN; ADC_POLICY_INTERPOLATION as the teacher (its update keys
 * its points by the bid it returned, which on a learner-driven day is not the bid the outcomes came from).
 * adc_engine_dagger_mask_fetch: out_tn [days recorded][N], 1 where the teacher's action was consumed (rows of plain teacher days
 * read 1); refused (ADC_ESTATE) when the record holds a day the learner collected. */
int adc_engine_dagger_days(adc_engine *e, int teacher_policy, int32_t days, float budget, float beta);
int adc_engine_dagger_mask_fetch(adc_engine *e, uint8_t *out_tn);
/* host twin (adc_shims.cpp) of the coin: 1 when the teacher's action is consumed */
int adc_dagger_coin_host(uint64_t key, uint32_t tick, float beta);

/* IMITATION is an add-on to a single-learner adc_engine_pg_init trainer: it shares its theta, Adam moments, lr, max_grad_norm and
 * minibatch_envs, so the cloned policy is the very theta adc_engine_pg_update goes on training, and the value network arrives
 * fitted to the teacher's returns.  adc_engine_im_advantages: the discounted returns of the teacher's rewards (GAE with lambda 1
 * under the trainer's gamma and reward_scale, no normalisation), the moving scale ma updated once over all recorded samples, the
 * call's scale c; adv_tn / ret_tn [T][N] may be NULL.  adc_engine_im_minibatch: one gradient of -(w logp(teacher action)) + the
 * value loss over every recorded day of an env range and one optimiser step; adc_engine_im_update: `epochs` times the contiguous
 * minibatches of minibatch_envs in ascending env order, the last epoch's statistics averaged (it does not compute the advantages:
 * adc_engine_im_advantages first).  Refused (ADC_ESTATE / ADC_EINVAL): without a single-learner trainer; with the KL or the
 * shuffle add-on or a running normaliser alive (and those are refused while imitation lives); with a record holding a day that is
 * not a teacher day ("the record holds days the learner collected"); a minibatch or update before adc_engine_im_advantages since
 * the last recorded day; beyond the LDS limit.  Imitation ends wherever the trainer ends. */
typedef struct adc_im_config {
    uint32_t struct_size;          /* sizeof(adc_im_config) */
    float beta;                    /* >= 0; 0: behaviour cloning (w = 1, no exp evaluated) */
    float vf_coef;                 /* >= 0; 0 drops the value loss */
    float w_max;                   /* > 0: the weight's cap; 0: none */
    double ma_start, ma_rate;      /* the moving scale: ma_start >= 0 (100), ma_rate in [0, 1] (1e-8) */
    int32_t train_log_std;         /* 0: dL/dlog_std = +0 (the free log_std stays the user's action scale) */
} adc_im_config;
typedef struct adc_im_stats {
    int64_t steps;                 /* optimiser steps taken so far (the trainer's count) */
    int64_t samples;               /* samples of the (last) minibatch */
    double policy_loss, value_loss, entropy;
    double logp;                   /* mean log-probability of the teacher's actions */
    double weight;                 /* mean w */
    double grad_norm;              /* before the clip */
    double explained_variance;     /* of the value function at collection against the teacher's returns */
} adc_im_stats;
int adc_im_config_check(const adc_im_config *cfg, const char **message);                /* host only */
int adc_engine_im_init(adc_engine *e, const adc_im_config *cfg);
int adc_engine_im_advantages(adc_engine *e, float *adv_tn, float *ret_tn);
int adc_engine_im_minibatch(adc_engine *e, int32_t env_begin, int32_t env_count, adc_im_stats *stats);
int adc_engine_im_update(adc_engine *e, int32_t epochs, adc_im_stats *stats);
/* ma and the number of advantages calls; theta, m, v and the steps are adc_engine_pg_state_get's */
int adc_engine_im_state_get(adc_engine *e, double *ma, int64_t *calls);
int adc_engine_im_state_set(adc_engine *e, double ma, int64_t calls);
/* host twins (adc_shims.cpp), the code the device runs.  adc_im_weight_host: one advantages call's scale and weights -
 * *ma (in: the state before, out: after), *c, w_s [count] from adv_s [count] (w_s may be NULL).  adc_im_grad_host: the gradient,
 * the law's ten sums and the statistics of `count` samples under the scale c, as adc_pg_grad_host */
int adc_im_weight_host(const adc_im_config *cfg, int64_t count, const float *adv_s, double *ma, float *c, float *w_s);
int adc_im_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_im_config *cfg, float c, const float *theta_q, int64_t count,
                     const float *obs_sd, const float *action_sa, const float *adv_s, const float *ret_s, const float *value_old_s, float *grad_q,
                     double *sums10, adc_im_stats *stats);

/* ---- off-policy training on the device: a replay ring, twin critics, TD3 (the law is csrc/adc_td3.h) --------------------------
 * The actor is the policy network given to adc_engine_mlp_init with the free log_std[A] head; its mean is TD3's deterministic
 * action, and the stochastic act mean + exp(log_std) * z is the exploration (set log_std = log(sigma); TD3 never trains it; a
 * value network is ignored).  Two Q networks on [x | an] - x the recorded network input, an the action, normalised when
 * adc_engine_td3_set_action_norm uploaded a shift and a scale - and target copies of the actor and of both critics live on the
 * device.  adc_engine_td3_store appends the record's days not yet stored to a ring of `capacity` transitions (x, a, r, done, x'),
 * adc_engine_td3_update takes critic updates on counter-addressed minibatches, every policy_delay-th followed by the actor's
 * step through critic 1's input gradient and the Polyak step of the targets; the new actor is written into the device's policy
 * layers (adc_engine_mlp_act, the next recorded day and adc_engine_mlp_get_params see it at once).  No transition leaves the
 * device.  Training draws from its own key alone: the envs' and the agents' streams do not move.  Flat orders: theta[P] as
 * adc_engine_mlp_get_params; psi[2 Qc] critic 1's layers (each W input-major, then b), then critic 2's
 * (adc_engine_td3_param_counts).  theta starts as the device's policy at adc_engine_td3_init; later adc_engine_mlp_set_layer
 * calls do not reach it (adc_engine_td3_state_set does).  The trainer does not survive adc_engine_mlp_init or
 * adc_engine_rollout_enable.  Refused (ADC_ESTATE / ADC_EINVAL, the engine stays usable): before adc_engine_mlp_init and its
 * uploads, a two-headed policy, without a record or without ADC_ROLLOUT_OBS, with a population active, with a policy-gradient
 * trainer alive (and adc_engine_pg_init with this one alive), a store with no unstored day or after the envs were stepped or
 * reset outside the record, an update before every critic layer was uploaded or with an empty ring. */
enum adc_td3_optimiser { ADC_TD3_ADAM = 0, ADC_TD3_SGD = 1 };
typedef struct adc_td3_config {
    uint32_t struct_size;          /* sizeof(adc_td3_config) */
    float gamma;                   /* in [0, 1] */
    float tau;                     /* in (0, 1]: the targets' Polyak rate */
    int32_t policy_delay;          /* >= 1: critic updates per actor step */
    float target_noise;            /* >= 0: the smoothing noise's standard deviation */
    float target_noise_clip;       /* >= 0 */
    float action_lo, action_hi;    /* hi > lo: the target action is clamped to [lo, hi] */
    float reward_scale;            /* finite, != 0 */
    int32_t batch_size;            /* 1 .. 2^20 */
    int32_t capacity;              /* 1 .. 2^30 transitions */
    int32_t n_critic_layers;       /* 1..4 */
    int32_t critic_widths[4];      /* outputs of each critic layer; hidden ones <= 256, the last is 1 */
    float actor_lr, critic_lr;     /* >= 0 */
    float beta1, beta2, eps;       /* Adam: 0 <= beta < 1, eps > 0 */
    int32_t optimiser;             /* adc_td3_optimiser */
    float max_grad_norm;           /* > 0: clip each gradient's global norm; 0: off */
    uint64_t seed;                 /* of the batches and the target noise; 0: the engine's seed */
} adc_td3_config;
typedef struct adc_td3_stats {
    int64_t updates;               /* critic updates taken so far */
    int64_t actor_steps;           /* actor (and target) steps taken so far */
    int64_t buffer_size;           /* transitions in the ring */
    int64_t samples;               /* batch elements of an update */
    double critic_loss;            /* of the call's last update: the sum of the two critics' mean 0.5 (Q - y)^2 */
    double q1_mean, q2_mean, y_mean;
    double actor_loss;             /* -mean Q1(x, mu(x)) of the call's last actor step (0 when it took none) */
    double critic_grad_norm;       /* before the clip */
    double actor_grad_norm;        /* of the call's last actor step, before the clip (0 when it took none) */
} adc_td3_stats;
int adc_engine_td3_init(adc_engine *e, const adc_td3_config *cfg);
/* one Linear layer of critic 0 or 1: weights_in_out [n_in][n_out] row-major, bias [n_out].  The targets do not follow until
 * adc_engine_td3_sync_targets */
int adc_engine_td3_set_critic_layer(adc_engine *e, int32_t critic, int32_t layer, const float *weights_in_out, const float *bias_out);
/* an[a] = (action[a] - shift_a[a]) * scale_a[a] for the critics' action inputs; without this call an = action */
int adc_engine_td3_set_action_norm(adc_engine *e, const float *shift_a, const float *scale_a);
/* bounded TD3 (csrc/adc_td3.h "bounded"), the learner of the bounded act (adc_engine_mlp_set_bounds): the critics read the ring's
 * action n in [-1, 1] as stored, the target action is clamp(tanh(mu') + clipped noise, -1, 1) - target_noise and
 * target_noise_clip are in units of the half-range, as Fujimoto's 0.2 / 0.5 are - and the actor's gradient goes through
 * tanh(mu).  Everything else (store, batch, noise addresses, critic step, Polyak, statistics, prioritised replay, n-step returns,
 * the running normalisers, the observation history) is what it was.  bounded = 0: back.  Refused with ADC_ESTATE: without the
 * bounded act, with an action normalisation uploaded (and adc_engine_td3_set_action_norm is refused afterwards), with action_lo /
 * action_hi set, and while the ring holds transitions.  adc_engine_td3_store and adc_engine_td3_update are refused while the
 * act and the learner disagree.  A new adc_engine_td3_init starts unbounded.  adc_engine_td3_pop_set_bounded: the same for a
 * population, all members at once; adc_engine_td3_get_bounded: of either. */
int adc_engine_td3_set_bounded(adc_engine *e, int32_t bounded);
int adc_engine_td3_pop_set_bounded(adc_engine *e, int32_t bounded);
int adc_engine_td3_get_bounded(adc_engine *e, int32_t *bounded);
/* host twins of the bounded law: adc_td3_target_host and adc_td3_actor_grad_host without an action normalisation, under it */
int adc_td3_bounded_target_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, uint64_t seed, int64_t update,
                                const float *theta_target_p, const float *psi_target_q, int32_t count, const float *x2_bd, const float *r_b,
                                const uint8_t *done_b, float *y_b);
int adc_td3_bounded_actor_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, const float *theta_p,
                                    const float *psi_q, int32_t count, const float *x_bd, float *grad_p, double *sums2);
/* the target actor and the target critics become copies of the actor and the critics */
int adc_engine_td3_sync_targets(adc_engine *e);
/* the record's days not yet stored, into the ring; *stored (may be NULL): the transitions appended */
int adc_engine_td3_store(adc_engine *e, int64_t *stored);
int adc_engine_td3_buffer_info(adc_engine *e, int64_t *size, int64_t *written, int64_t *capacity);
/* `count` slots from `slot` on (inside [0, size)): x [count][D], a [count][A], r [count], done [count] (bytes), x2 [count][D]; any
 * pointer may be NULL */
int adc_engine_td3_buffer_fetch(adc_engine *e, int64_t slot, int64_t count, float *x, float *a, float *r, uint8_t *done, float *x2);
/* the same arrays into the slots from `slot` on (inside [0, capacity)), then written = `written` (>= slot + count: the ring then
 * holds min(written, capacity) transitions): a resumed run, or a known buffer */
int adc_engine_td3_buffer_load(adc_engine *e, int64_t slot, int64_t count, const float *x, const float *a, const float *r, const uint8_t *done,
                               const float *x2, int64_t written);
/* the ring slots update number `update` reads at the ring's current size: idx_b [batch_size] (adc_engine_td3_batch_size) */
int adc_engine_td3_batch_size(adc_engine *e, int32_t *batch_size);
int adc_engine_td3_batch_indices(adc_engine *e, int64_t update, int32_t *idx_b);
/* `updates` >= 1 critic updates (and the actor steps that fall among them); stats may be NULL */
int adc_engine_td3_update(adc_engine *e, int32_t updates, adc_td3_stats *stats);
int adc_engine_td3_param_counts(adc_engine *e, int64_t *actor_p, int64_t *critics_2qc);
/* theta, target theta [P]; psi, target psi [2 Qc]; the Adam moments of theta [P] and of psi [2 Qc]; the counters: with the ring
 * (adc_engine_td3_buffer_fetch / _load) a resumed run continues bit for bit (get: any pointer may be NULL) */
int adc_engine_td3_state_get(adc_engine *e, float *theta_p, float *psi_q, float *theta_target_p, float *psi_target_q, float *m_theta_p,
                             float *v_theta_p, float *m_psi_q, float *v_psi_q, int64_t *updates, int64_t *actor_steps);
int adc_engine_td3_state_set(adc_engine *e, const float *theta_p, const float *psi_q, const float *theta_target_p, const float *psi_target_q,
                             const float *m_theta_p, const float *v_theta_p, const float *m_psi_q, const float *v_psi_q, int64_t updates,
                             int64_t actor_steps);

/* ---- soft actor-critic on the device (parts/kernel_sac.inc; the law is csrc/adc_sac.h) --------------------------------------------
 * One learner over the two-headed policy (2A outputs: means, then log-stds) with clamp_log_std on and the squashed action set
 * (adc_engine_mlp_set_squash): the env is given lo + half (tanh(u) + 1), the record and the ring keep u, and the critics' action
 * input is t = tanh(u) in [-1, 1].  Two Q networks on [x | t] and their target copies live on the device; there is no target
 * actor.  adc_engine_sac_store appends the record's days not yet stored to the ring (TD3's ring and store).  One update of
 * adc_engine_sac_update: the soft target y under the LIVE actor and the target critics; the critics' step; the actor's step on
 * the same batch through the smaller of the two updated critics, with the reparameterised gradient through both heads; the
 * temperature's step on log_alpha (alpha_lr > 0), taken by a kernel that writes the device cell the next update's kernels read,
 * so that an update needs no host round trip; every target_update_interval-th update the Polyak step of the target critics.
 * The new actor is written into the device's policy layers.  Training draws from the td3 key's stages 16, 20 and 21 alone: the
 * envs' and the agents' streams do not move.  Flat orders: theta[P], psi[2 Qc] as adc_engine_td3_*.
 * Without a norm clip a call of U updates only enqueues kernels - the Adam constants of step updates + 1 .. updates + U travel as
 * launch arguments of that step's kernels, so nothing is uploaded before the chain - and waits once, for the statistics; with
 * max_grad_norm > 0 each step fetches its norm.
 * SAC, TD3 and the policy-gradient trainers exclude each other (ADC_ESTATE), and adc_engine_obs_norm_init, _rew_norm_init,
 * _td3_norm_init and _pbt_init are refused over SAC.  Refused as well (ADC_ESTATE / ADC_EINVAL, the engine stays usable): a
 * free-head policy, clamp_log_std off, squash not set, no record or no ADC_ROLLOUT_OBS, a population or learners active, an update
 * with an empty ring or before every critic layer was uploaded, shapes whose activations do not fit 64 KB of LDS.  The trainer
 * does not survive adc_engine_mlp_init or adc_engine_rollout_enable. */
typedef struct adc_sac_config {
    uint32_t struct_size;          /* sizeof(adc_sac_config) */
    float gamma;                   /* in [0, 1] */
    float tau;                     /* in (0, 1]: the target critics' Polyak rate */
    int32_t target_update_interval;/* >= 1: updates per Polyak step */
    float init_alpha;              /* > 0, finite */
    float target_entropy;          /* finite (the usual choice: -(K + 1)) */
    float alpha_lr;                /* >= 0; 0: alpha stays init_alpha */
    float eps_sq;                  /* > 0: inside the squash correction's logarithm (1e-6) */
    float reward_scale;            /* finite, != 0 */
    int32_t batch_size;            /* 1 .. 2^20 */
    int32_t capacity;              /* 1 .. 2^30 transitions */
    int32_t n_critic_layers;       /* 1..4 */
    int32_t critic_widths[4];      /* outputs of each critic layer; hidden ones <= 256, the last is 1 */
    float actor_lr, critic_lr;     /* >= 0 */
    float beta1, beta2, eps;       /* Adam: 0 <= beta < 1, eps > 0 */
    int32_t optimiser;             /* adc_td3_optimiser */
    float max_grad_norm;           /* > 0: clip each network gradient's global norm; 0: off */
    uint64_t seed;                 /* of the batches and both noises; 0: the engine's seed */
} adc_sac_config;
typedef struct adc_sac_stats {
    int64_t updates;               /* updates taken so far */
    int64_t buffer_size;           /* transitions in the ring */
    int64_t samples;               /* batch elements of an update */
    double critic_loss;            /* of the call's last update: the sum of the two critics' mean 0.5 (Q - y)^2 */
    double q1_mean, q2_mean, y_mean;
    double actor_loss;             /* mean (alpha lp - min Q) of the call's last update */
    double logp_mean;              /* mean lp of the actor step: the entropy estimate is its negative */
    double alpha, log_alpha;       /* after the call's last update */
    double critic_grad_norm, actor_grad_norm;      /* before the clip */
} adc_sac_stats;
int adc_engine_sac_init(adc_engine *e, const adc_sac_config *cfg);
int adc_engine_sac_set_critic_layer(adc_engine *e, int32_t critic, int32_t layer, const float *weights_in_out, const float *bias_out);
int adc_engine_sac_sync_targets(adc_engine *e);
int adc_engine_sac_store(adc_engine *e, int64_t *stored);
int adc_engine_sac_buffer_info(adc_engine *e, int64_t *size, int64_t *written, int64_t *capacity);
int adc_engine_sac_buffer_fetch(adc_engine *e, int64_t slot, int64_t count, float *x, float *a, float *r, uint8_t *done, float *x2);
int adc_engine_sac_buffer_load(adc_engine *e, int64_t slot, int64_t count, const float *x, const float *a, const float *r, const uint8_t *done,
                               const float *x2, int64_t written);
/* the ring slots update number `update` reads at the ring's current size: idx_b [batch_size] (adc_engine_sac_batch_size) */
int adc_engine_sac_batch_size(adc_engine *e, int32_t *batch_size);
int adc_engine_sac_batch_indices(adc_engine *e, int64_t update, int32_t *idx_b);
/* `updates` >= 1 updates; stats may be NULL */
int adc_engine_sac_update(adc_engine *e, int32_t updates, adc_sac_stats *stats);
int adc_engine_sac_param_counts(adc_engine *e, int64_t *actor_p, int64_t *critics_2qc);
/* theta [P]; psi, target psi [2 Qc]; the Adam moments of theta [P] and of psi [2 Qc]; log_alpha3 = {log_alpha, its m, its v}; the
 * counter: with the ring a resumed run continues bit for bit (get: any pointer may be NULL) */
int adc_engine_sac_state_get(adc_engine *e, float *theta_p, float *psi_q, float *psi_target_q, float *m_theta_p, float *v_theta_p, float *m_psi_q,
                             float *v_psi_q, float *log_alpha3, int64_t *updates);
int adc_engine_sac_state_set(adc_engine *e, const float *theta_p, const float *psi_q, const float *psi_target_q, const float *m_theta_p,
                             const float *v_theta_p, const float *m_psi_q, const float *v_psi_q, const float *log_alpha3, int64_t updates);

/* ---- TD3 learner populations: M independent off-policy learners in lock-step on one engine ------------------------------------
 * Over learners (adc_engine_mlp_learners, M >= 1, the free log_std head): member m has its own actor (its learner's policy layers),
 * exploration sigma (its learner's log_std: adc_engine_mlp_set_learner_log_std, read by the next act), twin critics, target
 * networks, optimiser moments, adc_td3_config and replay ring of `capacity` transitions; it collects on its own envs
 * [m n, (m + 1) n), n = N / M, and all members store and update together, every kernel launch covering all of them: the
 * launches and host round trips of an update do not grow with M.  The law is csrc/adc_td3.h as it is: everything member m
 * computes - ring contents, batch indices, targets, both gradients, theta, psi, both targets, all four moment vectors,
 * statistics - is bit for bit what adc_engine_td3_* computes on an engine of n envs at env_id_base + m n with the same
 * parameter planes, engine seed, agent seeds, initial actor and critics, log_std and configuration.  A member's ring slot of
 * sample s = (t - t0) n + local env is (written + s) mod capacity; its td3 key is that of its own seed (0: the engine's); the
 * chunks of the float64 sums are 1024 consecutive batch elements of the member.  written, size, updates and actor_steps are
 * single counters: the members move together.
 * adc_td3_pop_config_check (host only): every configuration passes adc_td3_config_check; count is 1 (shared) or `members`;
 * members divides num_envs and is at most 65535; batch_size, capacity, n_critic_layers, critic_widths and policy_delay are
 * equal in all; every other field may differ per member.  The network shapes, the activation, the observation normalisation and
 * the critics' action normalisation are shared.  adc_engine_td3_pop_init needs learners, the free log_std head, a record with
 * ADC_ROLLOUT_OBS and no other trainer alive (ADC_ESTATE otherwise; adc_engine_td3_init keeps refusing an engine with
 * learners); every member's theta starts as its device policy; a refused allocation is ADC_ENOMEM and leaves the engine as it
 * was.  The trainer does not survive adc_engine_mlp_init, adc_engine_mlp_learners or adc_engine_rollout_enable.  With no
 * member clipping (max_grad_norm 0 in all) adc_engine_td3_pop_update only enqueues kernels - the optimiser constants of up to 64
 * updates go up in one copy in front of them - and ends with one copy of the statistics; when any member clips, all members'
 * squared norms come down in one copy per step and their scales go up in one. */
int adc_td3_pop_config_check(const adc_td3_config *cfgs, int32_t count, int32_t num_envs, int32_t members, const char **message);
int adc_engine_td3_pop_init(adc_engine *e, const adc_td3_config *cfgs, int32_t count);
/* as adc_engine_td3_set_critic_layer, for one member */
int adc_engine_td3_pop_set_critic_layer(adc_engine *e, int32_t member, int32_t critic, int32_t layer, const float *weights_in_out, const float *bias_out);
int adc_engine_td3_pop_set_action_norm(adc_engine *e, const float *shift_a, const float *scale_a);       /* shared by all members */
/* the member's targets become copies of its actor and critics; member -1: every member's */
int adc_engine_td3_pop_sync_targets(adc_engine *e, int32_t member);
/* the record's days not yet stored into every member's ring; *stored_per_member (may be NULL): the transitions each member appended */
int adc_engine_td3_pop_store(adc_engine *e, int64_t *stored_per_member);
int adc_engine_td3_pop_buffer_info(adc_engine *e, int64_t *size, int64_t *written, int64_t *capacity, int32_t *batch_size);   /* any may be NULL */
/* one member's ring: as adc_engine_td3_buffer_fetch / _load (load sets the one `written` all members share) */
int adc_engine_td3_pop_buffer_fetch(adc_engine *e, int32_t member, int64_t slot, int64_t count, float *x, float *a, float *r, uint8_t *done, float *x2);
int adc_engine_td3_pop_buffer_load(adc_engine *e, int32_t member, int64_t slot, int64_t count, const float *x, const float *a, const float *r,
                                   const uint8_t *done, const float *x2, int64_t written);
int adc_engine_td3_pop_batch_indices(adc_engine *e, int32_t member, int64_t update, int32_t *idx_b);
/* `updates` >= 1 critic updates of every member (and the actor steps that fall among them); stats_m[M] or NULL */
int adc_engine_td3_pop_update(adc_engine *e, int32_t updates, adc_td3_stats *stats_m);
int adc_engine_td3_pop_param_counts(adc_engine *e, int64_t *actor_p, int64_t *critics_2qc);      /* of one member */
/* one member's vectors as adc_engine_td3_state_get / _set; the counters are the population's (set: the last call's stand) */
int adc_engine_td3_pop_state_get(adc_engine *e, int32_t member, float *theta_p, float *psi_q, float *theta_target_p, float *psi_target_q,
                                 float *m_theta_p, float *v_theta_p, float *m_psi_q, float *v_psi_q, int64_t *updates, int64_t *actor_steps);
int adc_engine_td3_pop_state_set(adc_engine *e, int32_t member, const float *theta_p, const float *psi_q, const float *theta_target_p,
                                 const float *psi_target_q, const float *m_theta_p, const float *v_theta_p, const float *m_psi_q, const float *v_psi_q,
                                 int64_t updates, int64_t actor_steps);
/* a member's hyperparameters from the next update on (the shared fields may not change) */
int adc_engine_td3_pop_set_config(adc_engine *e, int32_t member, const adc_td3_config *cfg);
/* actor, critics, all targets and moments of src into dst on the device - with_ring: its ring too - and dst's stores rebuilt; dst
 * keeps its configuration, its envs and its log_std.  The primitive of population-based training (the scheduler: adc_engine_pbt_*) */
int adc_engine_td3_pop_copy(adc_engine *e, int32_t src, int32_t dst, int32_t with_ring);

/* ---- SAC learner populations: M independent soft actor-critic learners in lock-step on one engine ------------------------------
 * Over learners (adc_engine_mlp_learners, M >= 1) of the two-headed policy with clamp_log_std on and the learners' squash set
 * (adc_engine_mlp_learners_set_squash: the bounds are shared): member m has its own actor (its learner's policy layers), twin
 * critics, target critics, optimiser moments, temperature cell {log_alpha, m, v, alpha}, adc_sac_config and replay ring of
 * `capacity` transitions; it collects on its own envs [m n, (m + 1) n), n = N / M, and all members store and update together,
 * every kernel launch covering all of them: the launches and host round trips of a store or an update do not grow with M.  The
 * law is csrc/adc_sac.h as it is: everything member m computes - ring contents, batch indices, y, both gradients, theta, psi,
 * target psi, all moment vectors, the temperature cell, the statistics - is bit for bit what adc_engine_sac_* computes on an
 * engine of n envs at env_id_base + m n with the same parameter planes, engine seed, agent seeds, initial actor and critics,
 * squash bounds and configuration.  A member's ring slot of sample s = (t - t0) n + local env is (written + s) mod capacity; its
 * td3 key is that of its own seed (0: the engine's); the chunks of the float64 sums are 1024 consecutive batch elements of the
 * member.  written, size and updates are single counters: the members move together.
 * adc_sac_pop_config_check (host only): every configuration passes adc_sac_config_check (that check's own message); count is 1
 * (shared: only the first is read) or `members`; members divides num_envs and is at most 65535; batch_size, capacity,
 * n_critic_layers, critic_widths and target_update_interval are equal in all; every other field may differ per member.
 * adc_engine_sac_pop_init needs learners, the two-headed policy with the clamp on, the learners' squash, a record with
 * ADC_ROLLOUT_OBS and no other trainer alive (ADC_ESTATE otherwise, the engine stays usable); every member's theta starts as its
 * device policy; a refused allocation is ADC_ENOMEM and leaves the engine as it was.  adc_engine_obs_norm_init, _rew_norm_init,
 * _td3_norm_init and _pbt_init are refused over a SAC population (ADC_ESTATE; its scheduler is adc_engine_pbt_init_sac).  The trainer does not survive adc_engine_mlp_init,
 * adc_engine_mlp_learners or adc_engine_rollout_enable.  The optimiser constants of up to 64 updates - the critics', the actors'
 * and the temperatures' steps - go up in one copy in front of the chain: with no member clipping (max_grad_norm 0 in all)
 * adc_engine_sac_pop_update only enqueues kernels and ends with one copy of the statistics; when any member clips, all members'
 * squared norms come down in one copy per step and their scales go up in one.  A member with alpha_lr == 0 keeps its cell; the
 * temperatures' launch is left out only when every member has alpha_lr == 0. */
int adc_sac_pop_config_check(const adc_sac_config *cfgs, int32_t count, int32_t num_envs, int32_t members, const char **message);
int adc_engine_sac_pop_init(adc_engine *e, const adc_sac_config *cfgs, int32_t count);
/* as adc_engine_sac_set_critic_layer, for one member */
int adc_engine_sac_pop_set_critic_layer(adc_engine *e, int32_t member, int32_t critic, int32_t layer, const float *weights_in_out, const float *bias_out);
/* the member's target critics become copies of its critics; member -1: every member's */
int adc_engine_sac_pop_sync_targets(adc_engine *e, int32_t member);
/* the record's days not yet stored into every member's ring; *stored_per_member (may be NULL): the transitions each member appended */
int adc_engine_sac_pop_store(adc_engine *e, int64_t *stored_per_member);
int adc_engine_sac_pop_buffer_info(adc_engine *e, int64_t *size, int64_t *written, int64_t *capacity, int32_t *batch_size);   /* any may be NULL */
/* one member's ring: as adc_engine_sac_buffer_fetch / _load (load sets the one `written` all members share) */
int adc_engine_sac_pop_buffer_fetch(adc_engine *e, int32_t member, int64_t slot, int64_t count, float *x, float *a, float *r, uint8_t *done, float *x2);
int adc_engine_sac_pop_buffer_load(adc_engine *e, int32_t member, int64_t slot, int64_t count, const float *x, const float *a, const float *r,
                                   const uint8_t *done, const float *x2, int64_t written);
int adc_engine_sac_pop_batch_indices(adc_engine *e, int32_t member, int64_t update, int32_t *idx_b);
/* `updates` >= 1 updates of every member; stats_m[M] or NULL */
int adc_engine_sac_pop_update(adc_engine *e, int32_t updates, adc_sac_stats *stats_m);
int adc_engine_sac_pop_param_counts(adc_engine *e, int64_t *actor_p, int64_t *critics_2qc);      /* of one member */
/* one member's vectors as adc_engine_sac_state_get / _set, log_alpha3 its cell's {log_alpha, m, v}; the counter is the population's
 * (set: the last call's stands) */
int adc_engine_sac_pop_state_get(adc_engine *e, int32_t member, float *theta_p, float *psi_q, float *psi_target_q, float *m_theta_p,
                                 float *v_theta_p, float *m_psi_q, float *v_psi_q, float *log_alpha3, int64_t *updates);
int adc_engine_sac_pop_state_set(adc_engine *e, int32_t member, const float *theta_p, const float *psi_q, const float *psi_target_q,
                                 const float *m_theta_p, const float *v_theta_p, const float *m_psi_q, const float *v_psi_q,
                                 const float *log_alpha3, int64_t updates);
/* a member's hyperparameters from the next update on (the shared fields may not change; init_alpha is not read again: the
 * temperature cell is state) */
int adc_engine_sac_pop_set_config(adc_engine *e, int32_t member, const adc_sac_config *cfg);
/* actor, critics, target critics, all moments and the temperature cell of src into dst on the device - with_ring: its ring too -
 * and dst's stores rebuilt; dst keeps its configuration, its envs and its seed.  With adc_engine_sac_pop_set_config the primitive
 * of population-based training over SAC; the scheduler is adc_engine_pbt_init_sac (kind ADC_PBT_SAC), whose exploit is the batched
 * form of this call and whose explore also moves the temperature cell (adc_engine_pbt_init itself still refuses a SAC population) */
int adc_engine_sac_pop_copy(adc_engine *e, int32_t src, int32_t dst, int32_t with_ring);

/* ---- population-based training on the device: fitness, exploit, explore (the law is csrc/adc_pbt.h) ---------------------------
 * A scheduler (Jaderberg et al. 2017: truncation selection, copy, perturb) over a live learner population - adc_engine_pg_pop_*
 * (kind ADC_PBT_PG), adc_engine_td3_pop_* (kind ADC_PBT_TD3) or adc_engine_sac_pop_* (kind ADC_PBT_SAC, started by
 * adc_engine_pbt_init_sac); it goes whenever that trainer goes.  A round
 * (adc_engine_pbt_step) is, in order: the members' fitness (reduced from the rollout record's reward on the device, only M
 * doubles leave it; or fitness_m handed in), its smoothing, the plan (ranking, donor draw, explored values: on the host, from
 * those M doubles), the exploit (ONE batched copy of every replaced member from its donor: weights, optimiser moments, the
 * rebuild of the destination's stores; TD3: all four vectors, all four moment vectors and, with_ring, the ring), the explore
 * (every replaced member's new hyperparameters into the host-mastered member table, which goes up in one copy; TD3's sigma:
 * the destination's log_std from the donor's, in the log domain, inside the exploit's launch), round + 1.  SAC: the exploit covers
 * the actor's and the critics' vectors with their moments, the target critics' vector (there is no target actor), the temperature
 * cell and, with_ring, the ring - at most four launches, one more with the ring; the explored actor_lr, critic_lr, alpha_lr, tau and
 * target_entropy go into the member's adc_sac_config as adc_engine_sac_pop_set_config would put them (init_alpha is not touched: the
 * cell is state), and SAC's alpha is explored on the device: the destination's cell becomes {clamp(donor's log_alpha + log factor),
 * donor's m, donor's v, mlp_exp(new log_alpha)} - for a member with alpha_lr == 0 a search over the fixed temperature itself; with
 * alpha untuned the cell is the donor's verbatim.  The launches and host round trips of a round do not grow with M or
 * replace_count: one wait before the plan, one at the end.
 * Hyperparameter ids - PG: 0 lr, 1 ent_coef, 2 eps_clip, 3 vf_coef; TD3: 0 actor_lr, 1 critic_lr, 2 target_noise, 3 tau,
 * 4 sigma (lo / hi / the result's hp in log units; see adc_pbt_result); SAC: 0 actor_lr, 1 critic_lr, 2 alpha_lr, 3 tau, 4 alpha
 * (log units as sigma's), 5 target_entropy.  A replaced member keeps its envs, its agents' keys and ticks, its untuned
 * hyperparameters and (TD3, SAC) its seed; it gets its donor's smoothed fitness and (PG) step count.
 * adc_pbt_config_check (host only): struct_size; 2 <= members; 1 <= replace_count <= members / 2; 0 <= fitness_ema < 1; the
 * factors positive and finite, the log factors finite; tuned_mask inside the kind's ids; for every tuned id lo <= hi, both
 * inside what the trainer's own configuration check admits (so an explored configuration is always a legal one: learning rates,
 * coefficients and noises lo >= 0, tau lo > 0 and hi <= 1, PG's eps_clip hi < 1; TD3's sigma, SAC's alpha - both logarithms - and
 * SAC's target_entropy any sign); with_ring 0 for PG; kind 2 is unassigned.  Refused (the engine stays usable):
 * adc_engine_pbt_init without a PG or TD3 population trainer and adc_engine_pbt_init_sac without a SAC population trainer
 * (ADC_ESTATE: a solo trainer or another kind's population is none), either with a bad configuration (ADC_EINVAL); adc_engine_pbt_fitness and a step without fitness_m with no day recorded (ADC_ESTATE);
 * adc_engine_pbt_exploit with a destination that is also a source (ADC_EINVAL). */
enum adc_pbt_kind { ADC_PBT_PG = 0, ADC_PBT_TD3 = 1, ADC_PBT_SAC = 3 };     /* 2 is unassigned and refused */
typedef struct adc_pbt_config {
    uint32_t struct_size;          /* sizeof(adc_pbt_config) */
    int32_t replace_count;         /* q: the q worst members are replaced by copies of members among the q best */
    float fitness_ema;             /* in [0, 1): the smoothing's weight of the past; 0: none */
    float factor_lo, factor_hi;    /* > 0, finite: the two perturbation factors */
    float log_factor_lo, log_factor_hi;    /* their float32 logarithms (TD3's sigma and SAC's alpha move in the log domain) */
    uint32_t tuned_mask;           /* bit h: hyperparameter id h is explored */
    float lo[8], hi[8];            /* the explored value's bounds per id */
    int32_t with_ring;             /* TD3, SAC: the exploit copies the donor's ring too */
    uint64_t seed;                 /* of the donor draw and the factor bits; 0: the engine's seed */
} adc_pbt_config;
typedef struct adc_pbt_result {
    double fitness;                /* the round's fitness of the member */
    double smoothed;               /* after the round (a replaced member: its donor's) */
    int32_t rank;                  /* the round's ranking: 0 the worst */
    int32_t src;                   /* the donor the member was replaced from; -1: kept */
    float hp[8];                   /* the member's hyperparameters by id after the round; TD3's id 4: the log-domain shift its
                                      log_std got from its donor's before the clamp (0: kept); SAC's id 4: the same of its log_alpha */
} adc_pbt_result;
int adc_pbt_config_check(const adc_pbt_config *cfg, int32_t members, int32_t kind, const char **message);
int adc_engine_pbt_init(adc_engine *e, const adc_pbt_config *cfg);
/* the scheduler of kind ADC_PBT_SAC over the live adc_engine_sac_pop_init trainer (ADC_ESTATE without one); every call below then
 * serves it */
int adc_engine_pbt_init_sac(adc_engine *e, const adc_pbt_config *cfg);
/* fitness_m[M] float64 of the recorded days so far */
int adc_engine_pbt_fitness(adc_engine *e, double *fitness_m);
/* the batched copy alone: member m becomes a copy of member src_of_m[m] (src_of_m[m] == m or -1: kept), as adc_engine_pg_pop_copy
 * / adc_engine_td3_pop_copy / adc_engine_sac_pop_copy (with_ring from the configuration) would make it pair by pair, in a fixed
 * number of launches; no sigma or temperature shift is applied */
int adc_engine_pbt_exploit(adc_engine *e, const int32_t *src_of_m);
/* one round; fitness_m[M] may be NULL (the device's, from the record); result_m[M] may be NULL */
int adc_engine_pbt_step(adc_engine *e, const double *fitness_m, adc_pbt_result *result_m);
/* round and smoothed fitness [M]: a run resumed from them (with the trainer's own state) continues bit for bit (get: either may be NULL) */
int adc_engine_pbt_state_get(adc_engine *e, int64_t *round, double *smoothed_m);
int adc_engine_pbt_state_set(adc_engine *e, int64_t round, const double *smoothed_m);

/* ---- the running observation normaliser on the device (the law is csrc/adc_norm.h) ------------------------------------------
 * The mean and variance of the RAW observation, column by column, kept as (count, mean, M2) and merged batch by batch from the
 * rollout record's network inputs (one read of the record, back to raw space through the vectors the rows were collected
 * under); after every update the policy's shift / scale are float32(mean) and float32(1 / max(std, min_std)), written in place
 * where the policy kernel reads them.  What Stable-Baselines3's VecNormalize and RLlib's MeanStdFilter do around an env, without
 * the record leaving the device.  per_member: with learners active every learner has its own normaliser, fed from its own envs
 * in its own order (member m's result is bit for bit a single engine's of its envs), and its own [D] vectors, each starting as
 * the policy's; the act / step / bootstrap path then reads the env's member's.  `member` below is 0 for the shared normaliser.
 * An update consumes the recorded days [t0, T) not yet consumed (t0: the day count at the previous update, 0 after
 * adc_engine_rollout_reset and at the first init) and is ordered after the env groups' streams as adc_engine_pg_advantages is.
 * A trainer calls it AFTER its PPO / A2C update and before the next adc_engine_rollout_reset: the update's bootstrap value is
 * then evaluated under the vectors the record was collected with.  adc_engine_mlp_set_norm between two updates makes the days
 * recorded before it samples under the wrong vectors: reset the record first.
 * adc_obs_norm_config_check (host only): struct_size; min_std finite and > 0; count_cap >= 0 (0: no forgetting).
 * adc_engine_obs_norm_init is refused (the engine stays usable): before adc_engine_mlp_init and its uploads (ADC_ESTATE); a policy
 * initialised without normalisation (ADC_EINVAL); a current scale that is not finite or not > 0 (ADC_EINVAL); per_member without
 * learners (ADC_ESTATE); a TD3 trainer, single or population, alive (ADC_ESTATE: its ring holds inputs normalised by older
 * vectors - and adc_engine_td3_init / adc_engine_td3_pop_init are refused while a normaliser is alive).
 * adc_engine_obs_norm_update is refused (ADC_ESTATE): no record or no ADC_ROLLOUT_OBS; no day recorded since the last update or
 * adc_engine_rollout_reset.  The normaliser does not survive adc_engine_mlp_init, adc_engine_mlp_learners or
 * adc_engine_rollout_enable (the policy kernel is back to the policy's own vectors).  While it lives adc_engine_mlp_set_norm
 * keeps writing the shared vectors - every member's with per-member vectors - and leaves the running moments alone.
 * state_get / state_set: count, mean[D], M2[D] (float64), shift[D], scale[D] (float32) of one normaliser (get: any may be NULL);
 * a run resumed from them, together with the trainer's own state, continues bit for bit.
 * adc_engine_obs_norm_copy: adc_engine_pbt_exploit's convention (src_of_m[m] == m or -1: kept): every replaced member's count,
 * mean, M2, shift and scale become its donor's, in ONE launch whatever M is; a destination that is also a source is refused
 * (ADC_EINVAL), so is a shared normaliser (ADC_ESTATE). */
typedef struct adc_obs_norm_config {
    uint32_t struct_size;          /* sizeof(adc_obs_norm_config) */
    int32_t per_member;            /* one normaliser and one pair of vectors per learner (needs adc_engine_mlp_learners) */
    double min_std;                /* > 0, finite: the floor of the standard deviation (scale <= 1 / min_std) */
    int64_t count_cap;             /* > 0: the running count never exceeds it (M2 scaled down with it); 0: off */
} adc_obs_norm_config;
int adc_obs_norm_config_check(const adc_obs_norm_config *cfg, const char **message);
int adc_engine_obs_norm_init(adc_engine *e, const adc_obs_norm_config *cfg);
int adc_engine_obs_norm_update(adc_engine *e);
int adc_engine_obs_norm_state_get(adc_engine *e, int32_t member, int64_t *count, double *mean_d, double *m2_d, float *shift_d, float *scale_d);
int adc_engine_obs_norm_state_set(adc_engine *e, int32_t member, int64_t count, const double *mean_d, const double *m2_d, const float *shift_d,
                                  const float *scale_d);
int adc_engine_obs_norm_copy(adc_engine *e, const int32_t *src_of_m);
/* one update on the host: the same code as the device's (adc_norm.h).  x_sd [S][D]: the batch's (already normalised) rows in
 * the law's sample order; shift_d / scale_d hold the vectors the rows were collected under and receive the new ones; *count,
 * mean_d, m2_d hold the running moments and receive the merged ones. */
int adc_obs_norm_host(const adc_obs_norm_config *cfg, int64_t S, int32_t D, const float *x_sd, int64_t *count, double *mean_d, double *m2_d,
                      float *shift_d, float *scale_d);

/* ---- the running reward normaliser on the device (the law is csrc/adc_rew_norm.h) ----------------------------------------------
 * The variance of the discounted return, kept as (count, mean, M2) in float64 and merged batch by batch from the rollout record's
 * rewards; after every update the reward multiplier `scale` is float32(1 / max(std, min_std)), written in place where the GAE
 * kernel reads it: under a live normaliser adc_engine_pg_advantages / _pg_update (and the _pg_pop_ calls) compute
 * r = reward * reward_scale * scale, clipped to [-clip, clip] when clip > 0, and go on as before.  What Stable-Baselines3's
 * VecNormalize(norm_reward=True) does around an env, without the record leaving the device.  The discount is the trainer's own
 * gamma (adc_pg_config.gamma; under a population the env's member's, as in force when the update runs).  Every env carries its
 * running discounted return G across updates and rollouts; a day that ends an episode zeroes it after its sample, and so does
 * adc_engine_reset for the envs it resets.  per_member: every learner of a population has its own normaliser, fed from its own
 * envs in its own order (member m's result is bit for bit a single engine's of its envs); otherwise one is shared by all envs.
 * `member` below is 0 for the shared normaliser.
 * An update consumes the recorded days [t0, T) not yet consumed (t0: the day count at the previous update, 0 after
 * adc_engine_rollout_reset and at init), is three launches whatever the number of members is, synchronises nothing, and marks the
 * advantages stale.  A trainer calls it BEFORE its PPO / A2C update: the record's rewards are scaled by statistics that include
 * them.
 * adc_rew_norm_config_check (host only): struct_size; min_std finite and > 0; clip finite and >= 0 (0: off); count_cap >= 0.
 * adc_engine_rew_norm_init is refused (ADC_ESTATE, the engine stays usable): without a live PPO / A2C trainer (adc_engine_pg_init
 * or adc_engine_pg_pop_init: it needs their gamma); per_member without a learner population; while a TD3 trainer lives (and
 * adc_engine_td3_init / adc_engine_td3_pop_init are refused while a normaliser lives).
 * adc_engine_rew_norm_update is refused (ADC_ESTATE): no record; no day recorded since the last update or adc_engine_rollout_reset.
 * The normaliser does not survive adc_engine_pg_init, adc_engine_pg_pop_init, adc_engine_mlp_init, adc_engine_mlp_learners or
 * adc_engine_rollout_enable.  adc_engine_pg_pop_set_config keeps working: a changed gamma is the one the next update uses.
 * state_get / state_set: count, mean, M2 (float64), scale (float32) of one normaliser (get: any may be NULL); returns_get / _set:
 * the envs' carry G [N] (float64).  A run resumed from them, together with the trainer's own state, continues bit for bit.
 * adc_engine_rew_norm_copy: adc_engine_pbt_exploit's convention (src_of_m[m] == m or -1: kept): every replaced member's count,
 * mean, M2 and scale become its donor's, in ONE launch whatever M is; a destination that is also a source is refused
 * (ADC_EINVAL), so is a shared normaliser (ADC_ESTATE).  The carry is the envs' and is not copied. */
typedef struct adc_rew_norm_config {
    uint32_t struct_size;          /* sizeof(adc_rew_norm_config) */
    int32_t per_member;            /* one normaliser per learner (needs adc_engine_pg_pop_init) */
    double min_std;                /* > 0, finite: the floor of the standard deviation (scale <= 1 / min_std) */
    float clip;                    /* > 0: the normalised reward is clipped to [-clip, clip]; 0: off */
    int64_t count_cap;             /* > 0: the running count never exceeds it (M2 scaled down with it); 0: off */
} adc_rew_norm_config;
int adc_rew_norm_config_check(const adc_rew_norm_config *cfg, const char **message);
int adc_engine_rew_norm_init(adc_engine *e, const adc_rew_norm_config *cfg);
int adc_engine_rew_norm_update(adc_engine *e);
int adc_engine_rew_norm_state_get(adc_engine *e, int32_t member, int64_t *count, double *mean, double *m2, float *scale);
int adc_engine_rew_norm_state_set(adc_engine *e, int32_t member, int64_t count, double mean, double m2, float scale);
int adc_engine_rew_norm_returns_get(adc_engine *e, double *g_n);
int adc_engine_rew_norm_returns_set(adc_engine *e, const double *g_n);
int adc_engine_rew_norm_copy(adc_engine *e, const int32_t *src_of_m);
/* one update of one normaliser on the host: the same code as the device's (adc_rew_norm.h).  reward_tn, terminated_tn,
 * truncated_tn [days][num_envs]: the normaliser's envs' days not yet consumed; gamma_n [num_envs]: every env's discount; carry_n
 * [num_envs] holds the envs' running returns and receives the new ones; *count, *mean, *m2 hold the running moments and receive
 * the merged ones; *scale receives the new multiplier. */
int adc_rew_norm_host(const adc_rew_norm_config *cfg, int32_t days, int32_t num_envs, const float *gamma_n, const float *reward_tn,
                      const uint8_t *terminated_tn, const uint8_t *truncated_tn, int64_t *count, double *mean, double *m2, float *scale,
                      double *carry_n);
/* adc_pg_gae_host under a normaliser: scale_n [num_envs] is every env's multiplier, clip as adc_rew_norm_config's.  With every
 * scale 1 and clip 0 it gives adc_pg_gae_host's bits. */
int adc_pg_gae_norm_host(const adc_pg_config *cfg, int32_t days, int32_t num_envs, const float *reward_tn, const uint8_t *terminated_tn,
                         const uint8_t *truncated_tn, const float *value_tn, const float *bootstrap_n, const float *scale_n, float clip,
                         float *adv_tn, float *ret_tn);

/* ---- running observation and reward normalisers for the TD3 learners (the law is csrc/adc_td3_norm.h) ---------------------------
 * The replay ring outlives the statistics, so it may not depend on them.  While a normaliser with `observations` lives the rollout
 * record's obs rows are the RAW flat observation (zeros on an episode's first day) - the policy network itself is still fed
 * (x - shift) * scale - and so are the ring's x / x' rows: adc_engine_rollout_fetch, adc_engine_td3_buffer_fetch / _load (and the
 * _td3_pop_ ones) and a PBT round's ring copy carry raw rows.  The TD3 batch kernels normalise x and x' as they gather them, with
 * the learner's CURRENT vectors, and - with `rewards` - compute the target from r * reward_scale * scale, clipped to
 * [-rew_clip, rew_clip] when rew_clip > 0; the multiplier is read on the device, no host round trip lies between an update of the
 * normaliser and the next TD3 update.  Without `observations` the record and the ring hold network inputs as before; without
 * adc_engine_td3_norm_init every call launches the kernels it launched and computes the bits it computed.
 * The observation moments are those of the raw rows (count, mean[D], M2[D] in float64); after an update shift = float32(mean),
 * scale = float32(1 / max(std, obs_min_std)) are written in place where the policy kernel and the batch kernels read them.  The
 * reward moments are adc_rew_norm.h's (the variance of the discounted return, a per-env float64 carry G that a day ending an
 * episode and adc_engine_reset zero) with the TD3 learner's gamma - under a population the env's member's, as in force when the
 * update runs.  per_member: every learner of a TD3 population has its own normalisers (and its own [D] vectors, each starting as
 * the policy's), fed from its own envs in its own order: member m's result is bit for bit a single engine's of its envs.
 * `member` below is 0 for the shared normaliser.
 * adc_engine_td3_norm_update consumes the recorded days [t0, T) not yet consumed (its own cursor t0: 0 at init and after
 * adc_engine_rollout_reset), enqueues at most five launches whatever the number of members is and synchronises nothing; *samples
 * (may be NULL) receives the samples a normaliser consumed.  A trainer calls it after the store and BEFORE its TD3 updates: the
 * batch is scaled by statistics that include the newest days.
 * adc_td3_norm_config_check (host only): struct_size; observations or rewards nonzero; the min_std finite and > 0; the count_cap
 * >= 0 (0: no forgetting); rew_clip finite and >= 0 (0: off).
 * adc_engine_td3_norm_init is refused, the engine staying usable: without a live adc_engine_td3_init / _td3_pop_init trainer
 * (ADC_ESTATE); per_member without a TD3 population (ADC_EINVAL); `observations` on a policy initialised without normalisation
 * (ADC_EINVAL); a day recorded since adc_engine_rollout_reset or a transition in the ring (ADC_ESTATE: they hold network inputs).
 * adc_engine_td3_norm_update is refused (ADC_ESTATE) with no unconsumed day.  The normaliser ends with its trainer -
 * adc_engine_mlp_init, adc_engine_rollout_enable, a new adc_engine_td3_init / _td3_pop_init, and for a population's trainer
 * adc_engine_mlp_learners / adc_engine_mlp_population - and the record is back to network inputs.  A single-learner trainer
 * survives adc_engine_mlp_learners and adc_engine_mlp_population (its calls are refused while they are active) and so do its
 * normalisers: after adc_engine_mlp_learners(0) / _mlp_population(0) the run continues on its raw ring, bit for bit.  adc_engine_obs_norm_init / adc_engine_rew_norm_init keep refusing a TD3 trainer, and
 * adc_engine_pg_init is refused while one lives.  While the normaliser lives adc_engine_mlp_set_norm keeps writing the shared
 * vectors - every member's with per-member ones - and leaves the moments alone; with raw rings its effect on sampled rows is
 * immediate.
 * state_get / state_set: one normaliser's observation part (count, mean[D], M2[D], shift[D], scale[D]) and reward part (count,
 * mean, M2, scale); get: any may be NULL; set: the pointers of a part that does not live are not read; counts >= 0, scales finite and > 0, shift and the means
 * finite, M2 finite and >= 0 (ADC_EINVAL).  returns_get / _set: the
 * envs' carry G [N] (needs `rewards`).  A run resumed from them, the trainer's state and the ring continues bit for bit.
 * adc_engine_td3_norm_copy: adc_engine_pbt_exploit's convention (src_of_m[m] == m or -1: kept): every replaced member's moments,
 * vectors and multiplier become its donor's, in ONE launch whatever M is; a destination that is also a source is refused
 * (ADC_EINVAL), so is a shared normaliser (ADC_ESTATE).  The carry is the envs' and is not copied. */
typedef struct adc_td3_norm_config {
    uint32_t struct_size;          /* sizeof(adc_td3_norm_config) */
    int32_t observations, rewards; /* which parts live; at least one nonzero */
    int32_t per_member;            /* needs adc_engine_td3_pop_*: one normaliser per learner */
    double obs_min_std;            /* > 0, finite: the floor of a column's standard deviation */
    int64_t obs_count_cap;         /* > 0: the running count never exceeds it (M2 scaled down with it); 0: off */
    double rew_min_std;            /* > 0, finite: the floor of the discounted return's standard deviation */
    int64_t rew_count_cap;
    float rew_clip;                /* > 0: the normalised reward is clipped to [-rew_clip, rew_clip]; 0: off */
} adc_td3_norm_config;
int adc_td3_norm_config_check(const adc_td3_norm_config *cfg, const char **message);
int adc_engine_td3_norm_init(adc_engine *e, const adc_td3_norm_config *cfg);
int adc_engine_td3_norm_update(adc_engine *e, int64_t *samples);
int adc_engine_td3_norm_state_get(adc_engine *e, int32_t member, int64_t *obs_count, double *obs_mean_d, double *obs_m2_d, float *shift_d, float *scale_d,
                                  int64_t *rew_count, double *rew_mean, double *rew_m2, float *rew_scale);
int adc_engine_td3_norm_state_set(adc_engine *e, int32_t member, int64_t obs_count, const double *obs_mean_d, const double *obs_m2_d, const float *shift_d,
                                  const float *scale_d, int64_t rew_count, double rew_mean, double rew_m2, float rew_scale);
int adc_engine_td3_norm_returns_get(adc_engine *e, double *g_n);
int adc_engine_td3_norm_returns_set(adc_engine *e, const double *g_n);
int adc_engine_td3_norm_copy(adc_engine *e, const int32_t *src_of_member_m);
/* the host twins: the same code as the device's.  obs: one update of one normaliser's observation part from the batch's RAW rows
 * x_sd [S][D] in the law's sample order; *count, mean_d, m2_d hold the running moments and receive the merged ones, shift_d /
 * scale_d receive the new vectors.  rew: adc_rew_norm_host's arguments under cfg's rew_min_std / rew_count_cap (gamma_n: every
 * env's TD3 discount).  y_norm: y_b [count] = td3_y_norm of r_b, done_b and q_b (the smaller target critic's value) under td3's
 * gamma and reward_scale, the multiplier `scale` and `clip`; with scale 1 and clip 0 these are the plain TD3 target's bits. */
int adc_td3_norm_obs_host(const adc_td3_norm_config *cfg, int64_t S, int32_t D, const float *x_sd, int64_t *count, double *mean_d, double *m2_d,
                          float *shift_d, float *scale_d);
int adc_td3_norm_rew_host(const adc_td3_norm_config *cfg, int32_t days, int32_t num_envs, const float *gamma_n, const float *reward_tn,
                          const uint8_t *terminated_tn, const uint8_t *truncated_tn, int64_t *count, double *mean, double *m2, float *scale,
                          double *carry_n);
int adc_td3_y_norm_host(const adc_td3_config *td3, int32_t count, const float *r_b, const uint8_t *done_b, const float *q_b, float scale, float clip,
                        float *y_b);

/* ---- running observation and reward normalisers for the SAC learners (the law is csrc/adc_sac_norm.h) ---------------------------
 * The TD3 normalisers' contract on the soft actor-critic trainer (adc_engine_sac_init / _sac_pop_init): everything said above for
 * adc_engine_td3_norm_* holds with "SAC" for "TD3", and only the differences follow.  While a normaliser with `observations`
 * lives the record's obs rows and the ring's x / x' are RAW (adc_engine_sac_buffer_fetch / _load, the _sac_pop_ ones and a PBT
 * round's ring copy carry raw rows); the three SAC batch kernels normalise x and x' as they gather them with the learner's CURRENT
 * vectors - the live actor of the target and of the actor step, the critics, the target critics and every weight gradient see the
 * normalised row.  With `rewards` the target is sac_y_norm: r * reward_scale * scale, clipped to [-rew_clip, rew_clip] when
 * rew_clip > 0, plus gamma * (q - alpha * lp) * (1 - done).  The entropy term is NOT scaled: under a normalised reward
 * target_entropy and alpha trade entropy against a return of about unit standard deviation, not against the env's money scale.
 * The return scan's discount is adc_sac_config.gamma - under a population the env's member's, as in force when the update runs.
 * Without adc_engine_sac_norm_init every call launches the kernels it launched and computes the bits it computed.
 * adc_engine_sac_norm_init is refused, the engine staying usable: without a live adc_engine_sac_init / _sac_pop_init trainer
 * (ADC_ESTATE; a TD3 trainer is not one); per_member without a SAC population (ADC_EINVAL); `observations` on a policy initialised
 * without normalisation (ADC_EINVAL); a day recorded since adc_engine_rollout_reset or a transition in the ring (ADC_ESTATE).
 * The normaliser ends with its trainer - adc_engine_mlp_init, adc_engine_rollout_enable, a new adc_engine_sac_init / _sac_pop_init
 * (or _td3_init / _td3_pop_init), and for a population's trainer adc_engine_mlp_learners / adc_engine_mlp_population - and the record
 * is back to network inputs.  adc_engine_obs_norm_init, _rew_norm_init and _td3_norm_init keep refusing a SAC trainer; the
 * adc_engine_td3_norm_* calls do not see a SAC normaliser, and these do not see a TD3 one.  Prioritised replay works with it: the
 * priorities come from |d| of the normalised inputs and the normalised target, and the tree is not touched by the normaliser.
 * adc_engine_sac_pop_copy leaves the normalisers alone; adc_engine_sac_norm_copy (adc_engine_pbt_exploit's convention, ONE launch
 * whatever M is) carries the donors' moments, vectors and multiplier after a PBT round.
 * adc_sac_y_norm_host: y_b [count] = sac_y_norm of r_b, done_b, q_b (the smaller target critic's value) and lp_b (log pi of the
 * next action) under sac's gamma and reward_scale, the temperature `alpha`, the multiplier `scale` and `clip`; with scale 1 and
 * clip 0 these are the plain SAC target's bits.  The moments' host twins are adc_td3_norm_obs_host / adc_td3_norm_rew_host. */
typedef struct adc_sac_norm_config {
    uint32_t struct_size;          /* sizeof(adc_sac_norm_config) */
    int32_t observations, rewards; /* which parts live; at least one nonzero */
    int32_t per_member;            /* needs adc_engine_sac_pop_*: one normaliser per learner */
    double obs_min_std;            /* > 0, finite: the floor of a column's standard deviation */
    int64_t obs_count_cap;         /* > 0: the running count never exceeds it (M2 scaled down with it); 0: off */
    double rew_min_std;            /* > 0, finite: the floor of the discounted return's standard deviation */
    int64_t rew_count_cap;
    float rew_clip;                /* > 0: the normalised reward is clipped to [-rew_clip, rew_clip]; 0: off */
} adc_sac_norm_config;
int adc_sac_norm_config_check(const adc_sac_norm_config *cfg, const char **message);
int adc_engine_sac_norm_init(adc_engine *e, const adc_sac_norm_config *cfg);
int adc_engine_sac_norm_update(adc_engine *e, int64_t *samples);
int adc_engine_sac_norm_state_get(adc_engine *e, int32_t member, int64_t *obs_count, double *obs_mean_d, double *obs_m2_d, float *shift_d, float *scale_d,
                                  int64_t *rew_count, double *rew_mean, double *rew_m2, float *rew_scale);
int adc_engine_sac_norm_state_set(adc_engine *e, int32_t member, int64_t obs_count, const double *obs_mean_d, const double *obs_m2_d, const float *shift_d,
                                  const float *scale_d, int64_t rew_count, double rew_mean, double rew_m2, float rew_scale);
int adc_engine_sac_norm_returns_get(adc_engine *e, double *g_n);
int adc_engine_sac_norm_returns_set(adc_engine *e, const double *g_n);
int adc_engine_sac_norm_copy(adc_engine *e, const int32_t *src_of_member_m);
int adc_sac_y_norm_host(const adc_sac_config *sac, int32_t count, const float *r_b, const uint8_t *done_b, const float *q_b, const float *lp_b, float alpha,
                        float scale, float clip, float *y_b);

/* ---- prioritised replay for the TD3 and SAC learners (the law is csrc/adc_per.h) --------------------------------------------------
 * An add-on of the live adc_engine_td3_init / _sac_init / _td3_pop_init / _sac_pop_init trainer: the batch of an update is drawn in
 * proportion to the slots' priorities from a radix-64 sum tree that lives on the device next to the ring (one tree, one `top` and
 * one set of batch buffers per member of a population, one configuration for all), the critics' output deltas and loss pieces are
 * weighted by the batch's importance weights w_b in (0, 1] (normalised by the batch's largest weight, not the buffer's), and after
 * the critics' pass the sampled slots' leaves become pa(0.5 (|d_1| + |d_2|) + eps) - the maximum over the batch elements that drew
 * the slot - and the nodes on their paths are rebuilt from their children.  The actor's step, the temperature's and the other
 * statistics are unweighted.  A transition written by *_store or *_buffer_load gets leaf = top, the largest leaf any update has
 * written (1 at init).  An update enqueues 4 + L launches more than without the add-on (sample, weights, priorities, leaves, one
 * rebuild per level; L = ceil(log64 capacity) >= 1), whatever the batch size and the number of members are, and waits for nothing;
 * a store 1 + L per contiguous slot range (two when the ring wraps).  Without adc_engine_replay_prio_init every call launches the
 * kernels it launched and computes the bits it computed.
 * adc_replay_prio_config_check (host only): struct_size; alpha and beta in [0, 1]; eps > 0 and finite; cap > eps and finite.
 * adc_engine_replay_prio_init needs a live TD3 or SAC trainer, solo or population (ADC_ESTATE otherwise); a ring that already
 * holds transitions is fine: its slots get leaf 1.  A second init starts over.  _set_beta (the host's annealing schedule) takes
 * effect from the next update enqueued.  _info: member's total (the root) and top.  _fetch: the leaves of the slots [slot, slot +
 * count) inside [0, size).  _load: those leaves from the host (finite and > 0, ADC_EINVAL otherwise) and `top` (finite, > 0); the
 * nodes are rebuilt.  _batch: what update number `update` would draw from the tree as it stands: the slots idx_b [B] and the
 * weights weight_b [B] (either may be NULL); ADC_ESTATE on an empty ring.  `member` is 0 for a solo trainer.
 * While the add-on lives adc_engine_{td3,sac,td3_pop,sac_pop}_batch_indices are refused (ADC_ESTATE): they speak for the uniform
 * law.  The add-on ends with its trainer, under adc_engine_td3_norm_init's rules.  Copies that carry the ring carry the member's
 * leaves, nodes and top: adc_engine_td3_pop_copy / _sac_pop_copy with with_ring != 0 and adc_engine_pbt_exploit with rings;
 * without the ring they leave them alone. */
typedef struct adc_replay_prio_config {
    uint32_t struct_size;          /* sizeof(adc_replay_prio_config) */
    float alpha;                   /* [0, 1]: the priorities' exponent; 0: every leaf is 1 (uniform over the stored slots) */
    float beta;                    /* [0, 1]: the importance weights' exponent; 0: every weight is 1 */
    float eps;                     /* > 0, finite: added to the error, and the floor of a priority */
    float cap;                     /* > eps, finite: the ceiling of a priority */
} adc_replay_prio_config;
int adc_replay_prio_config_check(const adc_replay_prio_config *cfg, const char **message);
int adc_engine_replay_prio_init(adc_engine *e, const adc_replay_prio_config *cfg);
int adc_engine_replay_prio_set_beta(adc_engine *e, float beta);
int adc_engine_replay_prio_info(adc_engine *e, int32_t member, double *total, float *top);
int adc_engine_replay_prio_fetch(adc_engine *e, int32_t member, int64_t slot, int64_t count, float *leaf);
int adc_engine_replay_prio_load(adc_engine *e, int32_t member, int64_t slot, int64_t count, const float *leaf, float top);
int adc_engine_replay_prio_batch(adc_engine *e, int32_t member, int64_t update, int32_t *idx_b, float *weight_b);
/* the host twins: the same code as the device's, on a tree over `capacity` slots built from leaf_c [capacity] (zeros past the
 * stored slots).  tree: nodes receives the levels 1 .. L one after the other, n_l = ceil(n_{l-1} / 64) values each (counts [7]
 * receives n_0 .. n_L, zeros after; either may be NULL); returns L, or a negative error.  descend: the slot a descent with m reaches.
 * sample: idx_b / weight_b of update `update` under the td3 key of `seed` (adc_td3.h) for a ring of `size` stored slots.
 * priority: pa_b [count] = pa(p) of the unweighted errors d1_b, d2_b.  leaf_update: leaf_c and *top after the batch's slots idx_b
 * took pa_b (the maximum over duplicates). */
int adc_per_tree_host(int64_t capacity, const float *leaf_c, double *nodes, int64_t *counts);
int adc_per_descend_host(int64_t capacity, const float *leaf_c, double m, int64_t *slot);
int adc_per_sample_host(const adc_replay_prio_config *cfg, int64_t capacity, int64_t size, const float *leaf_c, uint64_t seed, int64_t update, int32_t count,
                        int32_t *idx_b, float *weight_b);
int adc_per_priority_host(const adc_replay_prio_config *cfg, int32_t count, const float *d1_b, const float *d2_b, float *pa_b);
int adc_per_leaf_update_host(int64_t capacity, float *leaf_c, float *top, int32_t count, const int32_t *idx_b, const float *pa_b);

/* ---- n-step returns for the TD3 / SAC learners (csrc/adc_td3.h "n-step"; parts/nstep_api.inc) --------------------------------- */
/* An add-on to a live off-policy trainer, solo or population, in adc_engine_replay_prio_init's sense.  With a window of n days a
 * store writes, for the sample of recorded day t, r = R = r[t] + gamma r[t+1] + ... over at most n days (each term one product, one
 * sum), done = the last summed day's flag, x' = the observation m days on (the stored fragment's end: the row an act would read
 * now) and a per-slot bootstrap discount gn = gamma^m formed by m - 1 products; the targets read gn[slot] where they read gamma.  A
 * window is cut at the first day that ends an episode and at the end of the stored fragment [t0, t1): the last n - 1 days of every
 * store carry a shorter window, and their gn says so (no fixed gamma^n).  The normalisers' reward multiplier and clip apply to R.
 * Slot addressing, the counters, the batch, the noise and the priorities do not move; with n = 1 the ring and the targets are the
 * add-on-off bits.  Without adc_engine_replay_nstep_init every call launches the kernels it launched and computes the bits it
 * computed.
 * _init needs a live TD3 or SAC trainer (ADC_ESTATE otherwise) and n in 1..16 (ADC_EINVAL otherwise); a ring that already holds
 * transitions is fine: its slots get gn = their member's gamma, being one-step.  A second init changes the window from the next
 * store on.  n is shared by a population's members, gamma is each member's own.  _info: n, 0 while the add-on is off.  _fetch: gn of
 * the slots [slot, slot + count) inside [0, size); _load: those inside [0, capacity) from the host (finite and >= 0, ADC_EINVAL
 * otherwise), next to *_buffer_fetch / _load, which move R and done.  `member` is -1 or 0 for a solo trainer.
 * adc_engine_td3_pop_set_config, _sac_pop_set_config and a PBT round may change a member's gamma after it has stored: the stored
 * slots keep the R and gn they were stored with.  Copies that carry the ring carry gn (adc_engine_td3_pop_copy / _sac_pop_copy
 * with with_ring != 0, adc_engine_pbt_exploit with rings).  The add-on ends with its trainer. */
int adc_replay_nstep_check(int32_t n, const char **message);
int adc_engine_replay_nstep_init(adc_engine *e, int32_t n);
int adc_engine_replay_nstep_info(adc_engine *e, int32_t *n);
int adc_engine_replay_nstep_fetch(adc_engine *e, int32_t member, int64_t slot, int64_t count, float *gn);
int adc_engine_replay_nstep_load(adc_engine *e, int32_t member, int64_t slot, int64_t count, const float *gn);
/* the host twins: the same code as the device's.  nstep: the windows of every sample s = (t - t0) * N + env of the days [t0, t1) of
 * a record reward / term / trunc [T][N]: R, done, gn and m [(t1 - t0) N] (any may be NULL).  y_nstep: adc_td3_y_norm_host /
 * adc_sac_y_norm_host with a per-element bootstrap discount gn_b [count]; scale = 1 and clip = 0 give the plain target's bits. */
int adc_replay_nstep_host(int32_t n, float gamma, int32_t T, int32_t N, int32_t t0, int32_t t1, const float *reward, const uint8_t *term,
                          const uint8_t *trunc, float *R, uint8_t *done, float *gn, int32_t *m);
int adc_td3_y_nstep_host(const adc_td3_config *td3, int32_t count, const float *r_b, const uint8_t *done_b, const float *q_b, const float *gn_b,
                         float scale, float clip, float *y_b);
int adc_sac_y_nstep_host(const adc_sac_config *sac, int32_t count, const float *r_b, const uint8_t *done_b, const float *q_b, const float *lp_b,
                         const float *gn_b, float alpha, float scale, float clip, float *y_b);

/* ---- info["bidding_outcomes"] on demand (src/lib.rs:251-275, adcraft/gymnasium_kw_env.py:247-251) -------------------- */
/* The fused step kernels keep per-keyword totals, not the per-click lists the reference formats ('costs', 'revenues',
 * 'revenues_per_cost').  Every variate is addressed by (env key; index, stage, keyword, tick), so those lists can be
 * regenerated exactly, only when somebody reads them: this call walks one env-step once more, read-only, in the reference's
 * order (sub-timestep, keyword, auction; the budget walk in its floating point) and lists the paid clicks: keyword[i],
 * timestep[i], cost[i] (dollars), revenue[i] (dollars; -1 = the click did not convert).  steps_back = 1: env `env`'s LAST
 * step; k > 1: the k-th last - valid while no reset / tape replay lies in between, drift is off and the caller has not
 * changed the env's parameters since (the stream position is recomputed, the parameters are read as they stand).  *count =
 * paid clicks of the step (may exceed capacity: then only `capacity` are stored).  share_volume_k[K] (optional) = per
 * keyword, the auctions of the sub-timesteps that had an impression - the denominator combine_outcomes ends up with for
 * 'impression_share' (bidding_simulation.py:130-146).  `bids_k` and `budget` are that step's action for this env.
 * ADC_ESTATE when the step cannot be replayed. */
int adc_engine_outcomes_replay(adc_engine *e, int32_t env, int32_t steps_back, const float *bids_k, float budget, int64_t capacity,
                               int32_t *keyword, int32_t *timestep, double *cost, double *revenue, int64_t *count, int32_t *share_volume_k);
/* The same lists for a step given as a tape (parity mode: the variates the reference drew, adc_engine_step_replay): env `env`
 * is walked over `tape` (its volumes, per-env start offsets and lengths as for adc_engine_step_replay; the end cursors are not
 * written), read-only, with the keyword parameters as they stand.  This is how the lists are pinned against the reference's
 * own BiddingOutcomes (adcraft/bidding_simulation.py:10-38,124-147; tests/golden/g3_*.json, g8_env_episodes.json). */
int adc_engine_outcomes_replay_tape(adc_engine *e, int32_t env, const float *bids_k, float budget, const adc_tape *tape, int64_t capacity,
                                    int32_t *keyword, int32_t *timestep, double *cost, double *revenue, int64_t *count, int32_t *share_volume_k);

/* ---- standalone auction clearing (adcraft/synthetic_kw_helpers.py:116-180) ------------------------ */
/* other_bids: host double [n_auctions][n_bidders]; placements/costs: host, capacity n_auctions.
 * Returns the impression count in *impressions.  num_winners + n must be <= 32. */
int adc_nth_price_auction(int device_id, double bid, const double *other_bids, int32_t n_auctions, int32_t n_bidders,
                          int32_t n, int32_t num_winners, int32_t *impressions, int32_t *placements, double *costs);

/* ---- scalar entry points mirroring `adcraft.rust` (src/lib.rs, function by function) -------------- */
double adc_sigmoid(double x, double s, double t);                               /* src/lib.rs:79-83,290-294 */
double adc_clamp(double x, double lo, double hi);                               /* probify_float, :86-90 */
double adc_threshold_sigmoid(double p, double impression_thresh,
                             double impression_bid_intercept, double impression_slope);   /* :93-105 */
double adc_sum_f64(const double *x, int64_t n);                                 /* sum_array / sum_list, :108-116 */
int64_t adc_count_true(const uint8_t *x, int64_t n);                            /* sum_array_bool / sum_list_bool */
/* samplers: the reference draws from an unseeded thread_rng (src/lib.rs:25,61,75,320); these draw from a
 * Philox stream keyed by (seed, counter) so callers can be reproducible. */
uint64_t adc_nonneg_int_normal(double mean, double std, uint64_t seed, uint64_t counter);   /* :314-325 */
uint64_t adc_binomial(uint64_t n, double p, uint64_t seed, uint64_t counter);               /* :70-76 */
int adc_cost_create(double x, int64_t n, uint64_t seed, uint64_t counter, double *out_n);   /* :54-67 */
/* diagnostic: the word-space thresholds k_step_implicit_fast resolves a keyword's auctions with (adc_law.h
 * win_intervals): word w is a clicked win iff (w - out4[0]) < out4[1], an unclicked win iff (w - out4[2]) < out4[3]
 * (uint32 arithmetic) - equivalent, word for word, to sampling the competitor's bid and running the reference's
 * nth_price_auction env path on it (adcraft/synthetic_kw_helpers.py:116-180: win iff bid > competitor) */
int adc_auction_word_intervals(float bid, float cost_loc, float cost_scale, float buyside_ctr, uint32_t *out4);
/* diagnostic: the conservative BRACKETS of those two intervals that k_step_implicit_sparse classifies a sparse keyword's
 * auctions with (adc_law.h win_brackets): out8 = {outer c_lo, c_w, n_lo, n_w, inner c_lo, c_w, n_lo, n_w}; a word inside an
 * inner interval wins, a word outside the outer ones loses, the rest is resolved from the sampled competitor bid.
 * adc_check_win_brackets verifies inner <= exact <= outer for n keywords (brackets8 NULL: the host's own evaluation;
 * otherwise e.g. adc_debug_win_brackets_device's) and returns the number of violations (0 expected). */
int adc_auction_word_brackets(float bid, float cost_loc, float cost_scale, float buyside_ctr, uint32_t *out8);
int64_t adc_check_win_brackets(int64_t n, const float *bid, const float *cost_loc, const float *cost_scale, const float *buyside_ctr,
                               const uint32_t *brackets8, int64_t *first_bad, double *ambiguous_words);
/* diagnostic: the two bounds those intervals come from, W(target) = min{v in [0, 2^24] : signed cents of the competitor's bid at
 * the 24-bit uniform v >= target} (adc_law.h), for n (target, loc, scale) on the host.  adc_lower_bound_v_host is the kernels'
 * routine (a window from one table evaluation, three accepting evaluations, a neighbourhood, then the bisection); stage_n (may be
 * NULL) says where each bound was settled: 0 accepted, 1 neighbourhood, 2 bisection.  adc_lower_bound_v_bisect_host is the
 * verified-window bisection alone, the reference; whole_range_n (may be NULL): 1 where its window did not hold the bound.
 * adc_win_intervals_host: out4 of adc_auction_word_intervals for n keywords with the bid in cents, from either routine
 * (bisect != 0: the reference; stage_n then holds 1 where either bound's window failed). */
int adc_lower_bound_v_host(int64_t n, const int32_t *target_n, const float *loc_n, const float *scale_n, uint32_t *v_n, uint8_t *stage_n);
int adc_lower_bound_v_bisect_host(int64_t n, const int32_t *target_n, const float *loc_n, const float *scale_n, uint32_t *v_n,
                                  uint8_t *whole_range_n);
int adc_win_intervals_host(int64_t n, const int32_t *bid_cents_n, const float *cost_loc_n, const float *cost_scale_n,
                           const float *buyside_ctr_n, int32_t bisect, uint32_t *out4_n, uint8_t *stage_n);
/* diagnostic: what the dense budget-free pass hoists out of its per-auction stages (adc_law.h), on the host, next to the routines it
 * stands for.  adc_draw_folded_host: n Philox calls three ways, four words each - the plain draw, the draw from the folded
 * (tick ^ key >> 32) word, and that draw started from the keyword's half of round 1; all three must agree.
 * adc_proven_win_price_host: for n keywords (bid in cents), the competitor's price without its clamp against the clamped one at
 * values of the keyword's win range - all of them where the range has at most exhaustive_below, else `ends` at either end and
 * `samples` drawn with `seed` - and at the two end words of the clicked-win interval; returns how many differ (first_bad3 =
 * {keyword, value, route} of the first or -1s, checked = values compared; both may be NULL), negative on bad arguments. */
int adc_draw_folded_host(int64_t n, const uint64_t *key_n, const uint32_t *index_n, const uint32_t *stage_n, const uint32_t *keyword_n,
                         const uint32_t *tick_n, uint32_t *plain4_n, uint32_t *folded4_n, uint32_t *kw4_n);
int64_t adc_proven_win_price_host(int64_t n, const int32_t *bid_cents_n, const float *cost_loc_n, const float *cost_scale_n,
                                  const float *buyside_ctr_n, int64_t exhaustive_below, int32_t ends, int32_t samples, uint64_t seed,
                                  int64_t *checked, int64_t *first_bad3);
/* diagnostic: how the budget-free IMPLICIT pass deals one tile's auctions to its lanes, on the host (the schedule arithmetic the
 * kernel calls, csrc/adc_fast_schedule.h).  vol_k = the volumes of the tile's tile_kw (1..256) keywords; tile_index (>= 0) = env x
 * tiles per env + tile, which only rotates the parts of the item range among the four waves.  Every issue slot becomes a
 * row of seven int32 {pass, wave, round, lane, keyword, first auction, count}; an idle slot has keyword -1 and count 0.  Pass 0 = full
 * work items, 1 = the whole Philox calls of the keywords' tails, 2 = the partial calls (the last V mod 4 auctions).  Returns the
 * number of rows, of which the first `cap` are written (slots7 may be NULL with cap 0), or a negative adc_status.  totals2 (may be
 * NULL) = {wave-call-slots issued: Philox calls, one per wave that runs them; calls that hold at least one auction, over all
 * keywords - 64 of these fill a slot}; info2 (may be NULL) = {log2 of the work-item size, 1 if the tile uses word intervals}. */
int64_t adc_fast_schedule_host(const int32_t *vol_k, int32_t tile_kw, int32_t tile_index, int32_t *slots7, int64_t cap, int64_t *totals2,
                               int32_t *info2);
/* diagnostic: the keywords that pass deals no work to (adc_law.h fast_keyword_is_dead: both win intervals empty, a day of zeros
 * whatever the words are), on the host, for n keywords with the bid in dollars.  dead_n = 1 where the interval form says so;
 * out4_n (may be NULL) = the intervals.
 * wins2_n (may be NULL), two counts per keyword over the words 0, T - 1, T, 2^32 - 2 (T = the click threshold) and n_random words
 * drawn with `seed`: the wins by auction-by-auction resolution, and the wins by the intervals. */
int adc_fast_dead_keywords_host(int64_t n, const float *bid_n, const float *cost_loc_n, const float *cost_scale_n, const float *buyside_ctr_n,
                                int32_t n_random, uint64_t seed, uint8_t *dead_n, uint32_t *out4_n, int64_t *wins2_n);
/* diagnostic: whether that pass keeps a keyword-day's cost and revenue in one 64-bit accumulator (adc_law.h fast_money_packs), on the
 * host, for n keyword-days (volume, bid in dollars, revenue law).  packs_n = 1 where the predicate says so; bid_c_n = the bid in
 * cents; r_max_n = the revenue bound of one conversion in cents that the predicate multiplies, -1 where the bound in dollars is NaN,
 * infinite or 1e7 and more (never packs); rev (may be NULL with n_words 0) = the revenue in cents at each of `words`, [n][n_words];
 * *z_max_out (may be NULL) = the normal table's largest node. */
int adc_fast_money_packs_host(int64_t n, const int32_t *volume_n, const float *bid_n, const float *rev_mean_n, const float *rev_std_n,
                              const uint32_t *words, int32_t n_words, uint8_t *packs_n, int32_t *bid_c_n, int64_t *r_max_n, int32_t *rev,
                              float *z_max_out);
/* diagnostic: the keyword-days whose clicked wins that pass resolves without the revenue's upper clamp and with one compare for the
 * conversion (adc_law.h fast_keyword_plain: it packs, and its conversion threshold is below 2^32), on the host.  plain_n = 1 where
 * the predicate says so; t32_n / T_n = the conversion threshold saturated to 32 bits / as it is; rev_tab, rev_plain [n][n_words]
 * (may be NULL with n_words 0; written for plain laws only) = adc::revenue_cents_tab and the unclamped form at each of `words`;
 * rev_rmax2_n [n][2] (plain laws only) = money_to_cents and its unclamped form at the law's revenue bound in dollars; conv_bad_n =
 * how often `word < t32` differs from the 64-bit test over the words 0, T - 1, T, 2^32 - 2, 2^32 - 1 and n_random drawn with `seed`. */
int adc_fast_plain_tiles_host(int64_t n, const int32_t *volume_n, const float *bid_n, const float *rev_mean_n, const float *rev_std_n,
                              const float *sellside_ctr_n, const uint32_t *words, int32_t n_words, int32_t n_random, uint64_t seed,
                              uint8_t *plain_n, uint32_t *t32_n, uint64_t *T_n, int32_t *rev_tab, int32_t *rev_plain, int32_t *rev_rmax2_n,
                              int32_t *conv_bad_n);
/* diagnostic: the queue tag of a clicked win in that pass, out4 = {tag, byte offset of the keyword's accumulator, keyword, auction};
 * keyword_in_tile < 256, auction <= 2^20 */
int adc_fast_tag_host(uint32_t keyword_in_tile, uint32_t auction, uint32_t *out4);
/* diagnostic: the protocol of that pass's per-wave queue of clicked wins, on the host, for one wave and a sequence of n_masks (< 2^26)
 * pushes.  Push p writes the lanes of masks[p] behind the entries that wait, entry = p << 6 | lane (a slot no push has written holds
 * 0xFFFFFFFF); whenever 64 or more wait after a push, a drain reads the batch [0, 64), reads the 64 slots behind it, writes those to
 * [0, 64) with all 64 lanes, takes 64 off the fill and only then resolves the batch from what it read; what is left after the last
 * push is one partial batch.  write_first = 1 runs the wrong order instead, the write ahead of the batch read (0 = the kernel's).
 * entries = what the batches resolved, one batch after the other in lane order (the first `cap` are written; may be NULL with cap 0);
 * batches2 [batches][2] = {entries that waited when the batch started, entries it resolved} (the first batch_cap rows; may be NULL
 * with batch_cap 0); info3 (may be NULL) = {batches, entries pushed, the largest number that ever waited}.  Returns the number of
 * entries resolved, or a negative adc_status. */
int64_t adc_fast_queue_host(const uint64_t *masks, int64_t n_masks, int32_t write_first, uint32_t *entries, int64_t cap, int32_t *batches2,
                            int64_t batch_cap, int64_t *info3);
/* one keyword of the default constructor's keyword set, on the host: exactly what adc_engine_generate_explicit_keywords writes for
 * keyword `keyword` of an env whose Philox key is `key` (adc_engine_get_rng_state) - sample_random_keywords' law
 * (gymnasium_kw_utils.py:113-156); out8 in adc_param order */
int adc_sample_random_keyword(uint64_t key, uint32_t keyword, uint32_t serial, float *out8);
/* one EXPLICIT keyword's cached bid curve, on the host: the n_samples normals adc_engine_bid_curves_build draws for keyword
 * `keyword` of an env whose Philox key / tick are `key` / `tick` (adc_engine_get_rng_state), sorted, and the same point function
 * (adc_law.h explicit_curve_point) on `bid_grid`.  cpc is bit-identical to the device's; ir uses the host's exp.
 * z_mid2_out (may be NULL): the two middle normals z_lo, z_hi.  n_samples <= 2^20. */
int adc_explicit_curve_host(uint64_t key, uint32_t tick, int32_t keyword, int32_t n_samples, float impression_thresh, float a, float b,
                            const double *bid_grid, int32_t n_bids, double *ir_out, double *cpc_out, double *z_mid2_out);
/* one keyword's act of the interpolation agent, on the host: the same code as the device's (adc_interp.h).  The cache is given
 * as the device keeps it (interpolation points in ascending cents 1..300; every cpc cent also a clicks cent); u = the uniform
 * rng.choice uses.  Out: margin_out / cost_out [n_bids] over the whole grid (get_expected_profit_per_bid_from_cache), *index_out
 * (-1: no draw), *bid_out (0.01 without a draw) and *mass_out (nullable: np.sum of the acquisition function up to end_index) */
int adc_interp_act_host(float ave_rpc, int32_t num_rpc_obs, float ave_sctr, int32_t num_sctr_obs, double max_observed,
                        double profit_acquisition_threshold, double bid_step, const double *allowed_bids, int32_t n_bids,
                        int32_t n_clicks, const uint16_t *clicks_cent, const float *ave_clicks, int32_t n_cpc, const uint16_t *cpc_cent,
                        const double *ave_cpc, double u, double *margin_out, double *cost_out, double *bid_out, int32_t *index_out,
                        double *mass_out);
/* the cache key of a bid: float(bidstr(bid)) = round(float(float32 bid), 2) */
double adc_interp_key_host(float bid);
/* one env's act of the MLP policy, on the host: the same code as the device's (adc_mlp.h).  obs_d: the flat observation row
 * (NULL: zeros, the first day).  policy_w[l] / value_w[l]: [n_in][n_out] row-major as for adc_engine_mlp_set_layer.  Normals:
 * normals_a when given, else drawn from (agent_key, tick) unless cfg->deterministic.  Out (any may be NULL): mean_a, log_std_a,
 * action_a [A], *logp, *value, bids_k [K] (cent bids as the env gets them), *budget. */
int adc_mlp_act_host(const adc_mlp_config *cfg, int32_t num_keywords, const float *obs_d, const float *const *policy_w,
                     const float *const *policy_b, const float *const *value_w, const float *const *value_b, const float *shift_d,
                     const float *scale_d, const float *log_std_a, const float *normals_a, uint64_t agent_key, uint32_t tick,
                     float budget_override, float *mean_a, float *log_std_out_a, float *action_a, float *logp, float *value,
                     float *bids_k, float *budget);
/* the observation history's row law for one env on the host: the same code as the device's (adc_mlp.h).  frame0_d0 [5K+2]: the
 * raw flat observation an act on episode day `day` reads (NULL, or day 0: zeros); hist_hd0 [frames][5K+2], *last, *from: the env's history.
 * row_d [frames (5K+2)] receives the raw stacked row.  commit nonzero: an act (frame 0 is written to its slot, *last and *from
 * move); zero: a peek (nothing is written).  ADC_EINVAL: frames outside 1..8, day < 0, a NULL history or row. */
int adc_mlp_stack_row_host(int32_t num_keywords, int32_t frames, const float *frame0_d0, float *hist_hd0, int32_t *last, int32_t *from,
                           int32_t day, int32_t commit, float *row_d);
/* the recurrent policy on the host: the same code as the device's (adc_gru.h).
 * adc_gru_cell_host: one step of the cell, h_out_g = cell(x_in [n_in], h_g [G]) under wi_in_3g, bi_3g, wh_g_3g, bh_3g (input-major,
 * gate order r | z | n).  ADC_EINVAL: n_in < 1, G outside 1..256, a NULL pointer.
 * adc_mlp_act_recurrent_host: one env's act as adc_mlp_act_host, with the cell of width gru_width in front of the output layer:
 * policy_w / policy_b hold the L layers (the last one [G][P]), h_in_g the input state (NULL: zeros), h_out_g (nullable) receives
 * the new state.
 * adc_gru_state_host: the state rule for one env.  h_2g [2][G], *last, *from: the env's state; h_in_g [G] receives the input state
 * of an act on episode day `day`; h_new_g (NULL: a peek, nothing is written) is the new state that act commits: it goes to its
 * slot, and *last and *from move.  ADC_EINVAL: G outside 1..256, day < 0, a NULL state or h_in_g. */
int adc_gru_cell_host(int32_t n_in, int32_t gru_width, const float *x_in, const float *h_g, const float *wi_in_3g, const float *bi_3g,
                      const float *wh_g_3g, const float *bh_3g, float *h_out_g);
int adc_mlp_act_recurrent_host(const adc_mlp_config *cfg, int32_t num_keywords, int32_t gru_width, const float *obs_d,
                               const float *const *policy_w, const float *const *policy_b, const float *wi_in_3g, const float *bi_3g,
                               const float *wh_g_3g, const float *bh_3g, const float *const *value_w, const float *const *value_b,
                               const float *shift_d, const float *scale_d, const float *log_std_a, const float *normals_a,
                               uint64_t agent_key, uint32_t tick, float budget_override, const float *h_in_g, float *mean_a,
                               float *log_std_out_a, float *action_a, float *logp, float *value, float *bids_k, float *budget,
                               float *h_out_g);
int adc_gru_state_host(int32_t gru_width, int32_t day, float *h_2g, int32_t *last, int32_t *from, float *h_in_g, const float *h_new_g);
/* the evolution strategy on the host: the same code as the device's (adc_es.h).  `seed` is the effective seed (the
 * configuration's, or the engine's when that is 0).  noise: eps(pair, generation)[p0 .. p0 + n).  update: one generation's
 * shaping, gradient estimate and step on theta / m / v [n_params] in place from fitness_m[members]; `generation` is the one
 * whose noise the members carried (the state's generation before the update); grad_p (may be NULL) receives the estimate. */
int adc_es_config_check(const adc_es_config *cfg, const char **message);
int adc_es_noise_host(uint64_t seed, uint32_t pair, uint32_t generation, int64_t p0, int64_t n, float *eps_n);
int adc_es_update_host(const adc_es_config *cfg, uint64_t seed, int32_t members, int64_t n_params, const double *fitness_m, int64_t generation,
                       float *theta_p, float *m_p, float *v_p, float *grad_p);
/* policy-gradient training on the host: the same code as the device's (adc_pg.h).  gae: returns and advantages [T][N] from a
 * record's arrays and the bootstrap values.  param_count: the length Q of the flat order.  grad: the loss pieces and the flat
 * gradient grad_q of `count` samples handed in as arrays (obs_sd [count][D] the recorded network input, action_sa [count][A]);
 * sums10 (may be NULL) receives the law's ten sums, stats (may be NULL) the statistics.  step: the norm clip and one optimiser
 * step on theta / m / v [n_params] in place; steps_taken is the count before the step. */
int adc_pg_config_check(const adc_pg_config *cfg, const char **message);
int adc_pg_gae_host(const adc_pg_config *cfg, int32_t days, int32_t num_envs, const float *reward_tn, const uint8_t *terminated_tn,
                    const uint8_t *truncated_tn, const float *value_tn, const float *bootstrap_n, float *adv_tn, float *ret_tn);
int adc_pg_param_count_host(const adc_mlp_config *mlp, int32_t num_keywords, int64_t *count);
int adc_pg_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_pg_config *cfg, const float *theta_q, int64_t count,
                     const float *obs_sd, const float *action_sa, const float *logp_old_s, const float *adv_s, const float *ret_s,
                     const float *value_old_s, float *grad_q, double *sums10, adc_pg_stats *stats);
int adc_pg_step_host(const adc_pg_config *cfg, int64_t n_params, int64_t steps_taken, const float *grad_q, float *theta_q, float *m_q,
                     float *v_q);
/* adc_pg_grad_host under the KL penalty and the value-loss clip (adc_pg_kl.h): kl's vf_clip, the coefficient kl_coef (the
 * configuration's own is not read), the collecting distribution mean_old_sa [count][A] and ls_old ([count][A] when
 * ls_old_per_sample, else the vector [A]).  sums_kl2 (may be NULL) receives the chunked sums of the per-sample KL and of the
 * value-clipped flags, kl_stats (may be NULL) the statistics (kl_coef_next = kl_coef).  adapt: the coefficient after an update
 * whose last epoch's mean KL was kl_mean. */
int adc_pg_kl_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_pg_config *cfg, const float *theta_q, int64_t count,
                        const float *obs_sd, const float *action_sa, const float *logp_old_s, const float *adv_s, const float *ret_s,
                        const float *value_old_s, const adc_pg_kl_config *kl, float kl_coef, const float *mean_old_sa, const float *ls_old,
                        int32_t ls_old_per_sample, float *grad_q, double *sums10, double *sums_kl2, adc_pg_stats *stats,
                        adc_pg_kl_stats *kl_stats);
int adc_pg_kl_adapt_host(const adc_pg_kl_config *kl, float coef, double kl_mean, float *coef_next);
/* adc_pg_shuffle.h on the host: the order of n_s samples for `tick` under the shuffle key of `seed` (order_out [n_s]: position i
 * holds sample sigma(i)); whether a minibatch with approx_kl ends the update under target_kl (*stop 1 or 0) */
int adc_pg_shuffle_order_host(uint64_t seed, int64_t n_s, uint32_t tick, uint32_t *order_out);
int adc_pg_shuffle_stop_host(double approx_kl, float target_kl, int32_t *stop);
/* what the end of a minibatch decides before its optimiser step (adc_pg_shuffle.h: pg_decide - the code k_pg_decide of the queued
 * update runs on the device): from the minibatch's ten sums sums10 over `count` samples, cfg's max_grad_norm and target_kl
 * (>= 0, finite; 0: never stops, as without shuffled minibatches).  *evaluated 1 (a minibatch handed over is evaluated),
 * *stop 1 when approx_kl = sums10[3] / count exceeds 1.5 target_kl - then no step: *clip 0, *scale 1 - else *clip whether
 * max_grad_norm > 0 and *scale the norm clip's factor under grad_norm = sqrt(sums10[9]) (1 with the clip off).  Any of the four
 * outputs may be NULL. */
int adc_pg_decide_host(const adc_pg_config *cfg, float target_kl, const double *sums10, int64_t count, int32_t *evaluated, int32_t *stop,
                       int32_t *clip, float *scale);
/* off-policy training on the host: the same code as the device's (adc_td3.h).  `seed` is the effective seed (the configuration's,
 * or the engine's when that is 0).  The batch arrays hold the gathered elements in order: x_bd / x2_bd [count][D], a_ba [count][A].
 * shift_a / scale_a: the action normalisation, both NULL for none.  target: y_b [count] from the target actor theta_target_p and
 * the target critics psi_target_q.  critic_grad: grad_q [2 Qc] and sums6 (may be NULL) = the chunked sums of the two loss pieces,
 * Q1, Q2, y and of grad^2.  actor_grad: grad_p [P] and sums2 (may be NULL) = the chunked sums of Q1(x, mu(x)) and of grad^2.  The
 * optimiser step is adc_pg_step_host. */
int adc_td3_config_check(const adc_td3_config *cfg, const char **message);
int adc_td3_param_counts_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, int64_t *actor_p, int64_t *critic_qc);
int adc_td3_batch_indices_host(uint64_t seed, int64_t update, int64_t size, int32_t count, int32_t *idx_b);
int adc_td3_target_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, uint64_t seed, int64_t update,
                        const float *theta_target_p, const float *psi_target_q, const float *shift_a, const float *scale_a, int32_t count,
                        const float *x2_bd, const float *r_b, const uint8_t *done_b, float *y_b);
int adc_td3_critic_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, const float *psi_q,
                             const float *shift_a, const float *scale_a, int32_t count, const float *x_bd, const float *a_ba, const float *y_b,
                             float *grad_q, double *sums6);
int adc_td3_actor_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, const float *theta_p,
                            const float *psi_q, const float *shift_a, const float *scale_a, int32_t count, const float *x_bd, float *grad_p,
                            double *sums2);
int adc_td3_polyak_host(float tau, int64_t n, const float *param_n, float *target_n);
/* soft actor-critic on the host: the same code as parts/kernel_sac.inc runs (adc_sac.h).  `seed` is the effective seed; the batch
 * arrays hold the gathered elements in order (x_bd / x2_bd [count][D], u_ba [count][A] the ring's unsquashed actions).
 * logp: from a head's outputs (means, raw log-stds) and given normals: u, t = tanh(u) and lp.  target: y_b (and lp_b, may be NULL)
 * from the live actor theta_p and the target critics.  critic_grad: grad_q [2 Qc], sums6 as adc_td3_critic_grad_host.
 * actor_grad: grad_p [P] through the smaller critic; lp_b (may be NULL) [count]; sums4 (may be NULL) = the chunked sums of the
 * loss piece and of lp, of grad^2, and the number of elements that took critic 2.  alpha_step: one step of log_alpha (la3 = {log_alpha, m,
 * v}, updated in place) from the chunked sum of lp over count elements with steps_taken steps before it; *alpha receives
 * exp(log_alpha).  The networks' optimiser step is adc_pg_step_host. */
int adc_sac_config_check(const adc_sac_config *cfg, const char **message);
int adc_sac_param_counts_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_sac_config *cfg, int64_t *actor_p, int64_t *critic_qc);
int adc_sac_logp_host(const adc_mlp_config *mlp, int32_t num_keywords, float eps_sq, int32_t count, const float *mean_ba, const float *raw_ba,
                      const float *z_ba, float *u_ba, float *t_ba, float *lp_b);
int adc_sac_target_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_sac_config *cfg, uint64_t seed, int64_t update, float alpha,
                        const float *theta_p, const float *psi_target_q, int32_t count, const float *x2_bd, const float *r_b, const uint8_t *done_b,
                        float *y_b, float *lp_b);
int adc_sac_critic_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_sac_config *cfg, const float *psi_q, int32_t count,
                             const float *x_bd, const float *u_ba, const float *y_b, float *grad_q, double *sums6);
int adc_sac_actor_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_sac_config *cfg, uint64_t seed, int64_t update, float alpha,
                            const float *theta_p, const float *psi_q, int32_t count, const float *x_bd, float *grad_p, float *lp_b, double *sums4);
int adc_sac_alpha_step_host(const adc_sac_config *cfg, int64_t steps_taken, double lp_sum, int32_t count, float *la3, float *alpha);
/* the log_alpha adc_engine_sac_init starts from */
float adc_sac_log_alpha_init_host(float init_alpha);
/* the scheduler of population-based training on the host: the same code as adc_engine_pbt_step runs (adc_pbt.h).  `seed` is the
 * effective seed (the configuration's, or the engine's when that is 0).  fitness: fitness_m[members] from a record's reward
 * [days][num_envs].  plan: smoothed_m holds s of the rounds before (not read in round 0) and receives this round's s, before any
 * copy; rank_m, src_m (-1: kept) and bits_m (the replaced member's factor bits w.y, 0 for the others) receive the plan.  explore:
 * out_hp8 for a replaced member from its donor's values donor_hp8, its own values own_hp8 and its factor bits (TD3's id 4: one
 * log_std component). */
int adc_pbt_fitness_host(int32_t days, int32_t num_envs, int32_t members, const float *reward_tn, double *fitness_m);
int adc_pbt_plan_host(const adc_pbt_config *cfg, uint64_t seed, int32_t members, int64_t round, const double *fitness_m, double *smoothed_m,
                      int32_t *rank_m, int32_t *src_m, uint32_t *bits_m);
int adc_pbt_explore_host(const adc_pbt_config *cfg, int32_t kind, uint32_t bits, const float *donor_hp8, const float *own_hp8, float *out_hp8);
/* the checks adc_engine_mlp_init makes on a configuration for num_keywords keywords; *message (may be NULL) names the failure */
int adc_mlp_config_check(const adc_mlp_config *cfg, int32_t num_keywords, const char **message);
/* the law's own tanh (fn 0) and exp (fn 1) at one float32, and a sweep over every float32 in [lo, hi] against the host's float64
 * libm: out3 = {maximum absolute error, maximum error in float32 ulps of the exact value, |result| maximum}; violations4 =
 * {f(-x) != -f(x) (tanh only), f(x) < f(previous x), |tanh| > 1, NaN results}.  Returns the number of values swept. */
float adc_mlp_math_host(int32_t fn, float x);
/* the squashed action of adc_engine_mlp_set_squash on the host: out_a[a] from u_a[a] under lo_a / hi_a, count components */
int adc_mlp_squash_host(int32_t count, const float *u_a, const float *lo_a, const float *hi_a, float *out_a);
int64_t adc_mlp_math_sweep_host(int32_t fn, float lo, float hi, double *out3, int64_t *violations4);
/* the agent key adc_engine_mlp_init derives from a per-env seed */
uint64_t adc_mlp_agent_key_host(uint64_t seed);
/* ... and the one it derives without seeds, from the engine's seed and the env's global id (env_id_base + env) */
uint64_t adc_mlp_default_agent_key_host(uint64_t engine_seed, uint64_t global_env_id);
/* diagnostic: the stream's generator (Philox4x32, the stream's round count) evaluated on the device for n counters ctr4[n][4]
 * and keys key2[n][2] -> out4[n][4]; tests compare it with the CPU battery's generator (oracle/stream_battery.c) */
int adc_debug_philox_device(int device_id, int64_t n, const uint32_t *ctr4, const uint32_t *key2, uint32_t *out4);
/* diagnostic: the reference's float64 budget chain `remaining -= sum(costs)` (bidding_simulation.py:225) over n cell sums x, as the
 * budget-exact kernels evaluate it - 64 rounded subtractions at a time by an integer prefix scan inside the running value's binade
 * (parts/common.inc chain_subtract_wave) -> out2[0]; and by the plain chain of n rounded subtractions on the device -> out2[1].
 * The two are the same float64, bit for bit, for every input. */
int adc_debug_chain_device(int device_id, double r0, int64_t n, const double *x, double *out2);
/* counters of k_step_click_walk on the engine's device since the library was loaded (or the last call with reset != 0):
 * stats[0] env-steps walked, [1] handed to the row kernel because the click list overflowed, [2] because the campaign
 * stopped, [3] for another reason (budget <= 0, a keyword-day above 2^22 cents in metric mode).  Test / measurement aid. */
int adc_debug_walk_stats(adc_engine *e, int64_t stats[4], int reset);
/* env-days k_tail_or_flag handed to k_step_rest_of_day at once, without the row kernel (a budget that ran out within the first
 * cells of the previous day), by THIS engine since it was created (or the last call with reset != 0).  Test / measurement aid. */
int adc_debug_direct_days(adc_engine *e, int64_t *env_days, int reset);
int adc_debug_win_brackets_device(int device_id, int64_t n, const float *bid, const float *cost_loc, const float *cost_scale,
                                  const float *buyside_ctr, uint32_t *out8);

#ifdef __cplusplus
}
#endif
#endif /* ADCRAFT_ENGINE_H */
