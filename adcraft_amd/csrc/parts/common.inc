// common.inc - device view of the engine, wave helpers, the log table, drift
// (part of the single translation unit adc_engine.hip; see that file for the overview)

thread_local std::string g_err;

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) {                                                                           \
            return fail(_e == hipErrorOutOfMemory ? ADC_ENOMEM : ADC_EHIP,                                \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                               \
        }                                                                                                 \
    } while (0)

constexpr int kFastBlock = 256;   // lanes per workgroup = keywords per tile
constexpr int kChunk = 16;        // auctions per work item
constexpr int kWave = 64;
constexpr int kProfileRing = 2048;   // steps in flight between profile flushes
constexpr int kProfileMarks = 4;     // events per step: before fast | after fast | after exact/tail | after metric

// developer instrumentation (python adcraft_amd/build.py --timing): per-phase sums, read by adc_debug_read
#ifdef ADC_EXP_TIMING
__device__ unsigned long long g_dbg[16];
__device__ unsigned long long g_fdbg[256][8];       // k_step_implicit_fast, wave 0 of each workgroup, spread over 256 rows
#define FDBG_T() __builtin_amdgcn_s_memtime()
#define FDBG_ADD(i, x) fdbg[i] += (x)
__device__ unsigned long long g_fslots[256][2];     // k_step_implicit_fast, every wave: Philox calls issued in phase 2 | calls that hold an auction
#define FSLOT_ADD(i, x) fslots[i] += (x)
#else
#define FDBG_T() 0ull
#define FDBG_ADD(i, x) (void)0
#define FSLOT_ADD(i, x) (void)0
#endif

// an env whose budget-bound day k_step_exact_rows hands to k_step_rest_of_day: where the walk stands
struct RestState {
    long long R;              // cents left
    double r_d;               // the reference's float remaining_budget
    int row;                  // first sub-timestep not yet looked at
    int flags;                // bit 0: the fast pass skipped the env (hint 2 / 6), bit 1: few clicks (may list them), bit 2: parked by
                              // k_tail_or_flag before anything of the day was looked at, bit 3: the budget bound within the first cells of the
                              // day, bits 4..: the hint it came with
    long long pc;             // k_rest_walk's path: the day's profit in cents up to the hand-over (the observations are written there too)
};

// -------------------------------------------------------------------------------------------------
// device view of the engine (passed by value to kernels)
struct View {
    int N, K, model, max_days;
    int NP;                   // envs the parameter planes / metric_env planes are strided by: the engine's N.  (N < NP: the view of an env
                              // GROUP - envs [e0, e0 + N) of the engine, every per-env pointer below offset to e0, lists and counters its
                              // own - that launch_step runs on a stream of its own beside the other groups: host_api.inc group_view)
    double loss_threshold;
    float drift_vol, drift_ctr, drift_cvr;
    int drift_on;
    float imp_thresh;
    int auto_reset;
    int metrics_on;
    int max_bidders, num_winners;     // ADC_MODEL_IMPLICIT_GENERAL
    float participation_rate;
    // state
    float *params;            // [8][N][K]
    uint64_t *key;            // [N]
    uint32_t *tick;           // [N]
    int32_t *day;             // [N]
    int64_t *cum_cents;       // [N] IMPLICIT
    double *cum;              // [N] EXPLICIT
    uint8_t *drift_pending;   // [N]
    const uint32_t *drift_bits;   // [N][ceil(K/32)] the keywords that move at update_keywords(), bit k & 31 of word k >> 5 of the env's row
                                  // (whole words per env); null = every keyword (adc_engine_set_drift_mask)
    const float *drift_rate;      // [N][3] the env's drift magnitudes vol, ctr, cvr; null = drift_vol / drift_ctr / drift_cvr above
                                  // (adc_engine_set_env_drift)
    uint8_t *exact_hint;      // [N] the budget bound on the previous step (a scheduling hint, never a result).  IMPLICIT: 1 = the fast pass also
                              // lists its clicked wins for k_step_click_walk, 2 = skip the fast pass, the row kernel computes the env alone,
                              // 3 / 4 (within a step) = the fast pass ran and k_step_click_walk handed the env to the row kernel: because the
                              // list overflowed (2 from tomorrow) / for this day only (1 again tomorrow); 6 = skip the fast pass, k_tail_or_flag
                              // parks the env for k_step_rest_of_day at once (the budget ran out within the first cells yesterday).
                              // Other models: 0 / 1
    int *flag_list;           // [N] envs that need the exact pass this step (filled by k_tail_or_flag)
    int *flag_count;          // [2] its length, double-buffered by step parity
    int *flag_next;           // [2] ticket counter of the persistent k_step_exact_rows grid
    int *xover_list;          // [N] EXPLICIT envs k_step_explicit_rows left to the serial walker; IMPLICIT: the envs of k_step_click_walk
    int *xover_count;         // [2] its length, double-buffered by step parity
    int *retry_list;          // [N] EXPLICIT envs k_step_float_day left to k_step_explicit_rows
    int *retry_count;         // [2] its length, double-buffered by step parity; IMPLICIT: the ticket counter of k_step_click_walk
    // IMPLICIT, K <= 256: clicked wins of the fast pass, for envs whose budget bound on the previous step (k_step_click_walk)
    uint2 *click_rec;         // [N][25][click_cap] per sub-timestep (click_seg_offset): {keyword << 20 | auction index in its cell, price in cents}; allocated by the host when the first env asks for lists (click_count != null: the path exists)
    uint32_t *click_count;    // [N][24] records listed this step (may exceed click_cap: then that list is incomplete)
    uint32_t *click_tick;     // [N] tick + 1 of the step the lists belong to (0 = none)
    uint8_t *click_row_hint;  // [N] sub-timesteps <= this are listed completely, later ones only ...
    uint32_t *click_price_hint;   // [N] ... the clicks costing at most this many cents (what the walk can still need once the budget is ground down)
    int click_cap;
    // IMPLICIT, K <= 1024: what k_step_exact_rows parks for k_step_rest_of_day (retry_list holds the envs)
    RestState *rest_state;    // [N]; null = the path is off
    uint4 *rest_counts;       // [N][K] impressions, clicks, conversions so far; the day's volume
    long long *rest_cost, *rest_rev;   // [N][K] cents so far
    int *rest_count;          // [2] envs parked this step, double-buffered by step parity
    int *rest_next;           // [2] ticket counter of the persistent k_step_rest_of_day grid
    unsigned short *rest_table;   // [N][24][K]: the cells' first clicks, from k_step_rest_of_day<true> to k_rest_walk for an env with more marks than
                                  // its list holds (allocated once a budget binds; rest_marks != null: the pair of kernels, else one)
    unsigned int *rest_marks;     // [N][rest_marks_stride]: the same as a list, (row * K + keyword) << 16 | cents, in the reference's order
    int *rest_nmarks;             // [N]: entries of the list, or -1: read the table
    int rest_marks_cap;           // entries of an env's list in use: kRestMarks per 256 keywords (tests: fewer)
    int rest_marks_stride;        // ... and allocated
    long long *direct_budget;     // [N] hint 6: the budget (cents) of the day that earned it (a larger one goes through the row kernel again)
    int *direct_list;             // [N] envs k_tail_or_flag parked this step (k_step_rest_of_day<true, true>), counter / ticket by step parity
    int *direct_count, *direct_next;      // [2] each
    unsigned long long *direct_days;      // [1] env-days parked at once so far, of THIS engine (adc_debug_direct_days)
    int *direct_flag;             // host-visible word k_rest_walk sets when an env earns hint 6 (the host then launches that kernel too)
    int *binding_flag;        // host-visible word the row kernel sets when a budget binds (the host then launches k_step_rest_of_day too)
    int *flags_seen;          // [3] device-side copies of binding_flag / listing_flag / direct_flag (tell_host_once)
    int *listing_flag;        // host-visible word the kernels set when an env starts listing (the host then launches the listing variant)
    int click_list_max;       // an env goes on to list its clicked wins only if a day has at most this many (denser: the row kernel alone is faster)
    // per-step scratch
    double *gs_profit, *gs_spend;   // [N][K] IMPLICIT_GENERAL, a handful of envs (k_step_general_small): a keyword-day's profit and its positive costs; null otherwise
    int64_t *env_cost;        // [N] cents spent by the fast pass
    int64_t *env_profit;      // [N]
    // outputs
    int32_t *imp, *clk, *conv;   // [N][K]
    float *cost, *rev;           // [N][K]
    double *reward, *cum_profit; // [N]
    int32_t *day_out;            // [N]
    uint8_t *term, *trunc;       // [N]
    // metrics
    int64_t *metric_profit;      // [K]
    int64_t *metric_scalars;     // [8] (filled on read)
    int64_t *metric_env;         // [4][N] per-env running sums: profit cents, env steps, episodes, truncations
    // [N][K] running sum of keyword profit, cents (metric mode): a 32-bit word that every step reads and writes (8 B of traffic per
    // keyword-step; round 3 kept 64 bits: 16) and a 64-bit spill touched only if the word would overflow - metric_add / metric_total
    int32_t *metric_lo;
    int64_t *metric_hi;
    float *flat_obs;             // [N][5K+2] FlatArrayWrapper layout, written after every step when enabled
};

// the keyword's running profit sum += delta (exact for any delta: what does not fit the 32-bit word moves to the spill)
__device__ __forceinline__ void metric_add(const View &v, size_t o, long long delta)
{
    const long long s = (long long)v.metric_lo[o] + delta;
    if (s == (long long)(int)s) v.metric_lo[o] = (int)s;
    else { v.metric_hi[o] += s; v.metric_lo[o] = 0; }
}
__device__ __forceinline__ long long metric_total(const View &v, size_t o) { return v.metric_hi[o] + (long long)v.metric_lo[o]; }


// tell the host something once (a page-locked flag word): every later caller sees the device-side copy set and leaves the
// bus alone (thousands of workgroups storing to one host address per step cost more than the kernels they announce)
__device__ __forceinline__ void tell_host_once(int *host_flag, int *device_seen)
{
    if (__hip_atomic_load(device_seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
    if (atomicExch(device_seen, 1) == 0) __hip_atomic_store(host_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// click lists (k_step_click_walk): per env 25 segments of click_cap records - sub-timestep 0 takes two (it holds the remainder of
// the 24-way split, adcraft/bidding_simulation.py:151-167, i.e. up to 23 auctions per keyword more than the other rows)
constexpr int kClickSegments = adc::kTimesteps + 1;
__device__ __forceinline__ size_t click_seg_offset(const View &v, int env, int row)
{
    return ((size_t)env * kClickSegments + (row == 0 ? 0 : row + 1)) * (size_t)v.click_cap;
}
__device__ __forceinline__ unsigned int click_seg_cap(const View &v, int row) { return (unsigned int)(row == 0 ? 2 * v.click_cap : v.click_cap); }

__device__ __forceinline__ float &param_at(const View &v, int p, int env, int k)
{
    return v.params[((size_t)p * v.NP + env) * v.K + k];
}

__device__ __forceinline__ unsigned long long lanemask_lt()
{
    return (1ull << (threadIdx.x & 63)) - 1ull;
}

// ---- cross-lane sums by DPP (data-parallel primitives: the operand of a VALU instruction comes from another lane of the
// row / wave, no LDS traffic).  __shfl_* goes through ds_bpermute with ~6 VALU instructions of index arithmetic per step.
// dpp_ctrl encodings (GFX9): row_shr:n = 0x110 + n, row_bcast:15 = 0x142, row_bcast:31 = 0x143
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_or_zero(int x)
{
    return __builtin_amdgcn_update_dpp(0, x, CTRL, ROW_MASK, 0xF, false);      // lanes without a source (or masked rows) read 0
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ long long dpp_or_zero(long long x)
{
    const unsigned long long u = (unsigned long long)x;
    const unsigned int lo = (unsigned int)dpp_or_zero<CTRL, ROW_MASK>((int)(unsigned int)u);
    const unsigned int hi = (unsigned int)dpp_or_zero<CTRL, ROW_MASK>((int)(unsigned int)(u >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// inclusive prefix sum across the 64 lanes of a wave: Hillis-Steele inside each row of 16 (row_shr 1, 2, 4, 8), then the
// row totals carried over by the two broadcasts
template <typename T>
__device__ __forceinline__ T wave_scan(T x)
{
    x += dpp_or_zero<0x111, 0xF>(x);
    x += dpp_or_zero<0x112, 0xF>(x);
    x += dpp_or_zero<0x114, 0xF>(x);
    x += dpp_or_zero<0x118, 0xF>(x);
    x += dpp_or_zero<0x142, 0xA>(x);          // rows 1 and 3 += lane 15 of the row before
    x += dpp_or_zero<0x143, 0xC>(x);          // rows 2 and 3 += lane 31
    return x;
}
__device__ __forceinline__ long long wave_scan_i64(long long x) { return wave_scan<long long>(x); }
__device__ __forceinline__ int wave_scan_i32(int x) { return wave_scan<int>(x); }

// sum over the wave, in every lane (lane 63 of the scan, broadcast by v_readlane)
__device__ __forceinline__ int wave_sum_i32(int x) { return __builtin_amdgcn_readlane(wave_scan<int>(x), 63); }
__device__ __forceinline__ long long wave_sum_i64(long long x)
{
    const unsigned long long u = (unsigned long long)wave_scan<long long>(x);
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)u, 63);
    const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(u >> 32), 63);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// value of lane l's x in every lane; l must be wave-uniform (v_readlane_b32 x 2)
__device__ __forceinline__ double readlane_f64(double x, int l)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)u, l);
    const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(u >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ long long readlane_i64(long long x, int l)
{
    const unsigned long long u = (unsigned long long)x;
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)u, l);
    const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(u >> 32), l);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// ((((r - x_0) - x_1) - ...) - x_63) in IEEE float64, every difference rounded, left to right - the reference's
// `remaining_budget -= sum(costs)` chain over the cells of a row (adcraft/bidding_simulation.py:225) - WITHOUT the 64 dependent
// subtractions (round 4 ran them one v_readlane pair and one v_add_f64 at a time: the single most expensive piece of a budget-bound
// step - removing it, wrongly, took 88 us off cfg2's 525).  While the running value stays inside its binade [2^E, 2^(E+1)) it is an
// integer M in [2^52, 2^53) times u = ulp = 2^(E-52), and subtracting x = (A + f) u, 0 <= f < 1, rounds to (M - A) u if f < 1/2 and to
// (M - A - 1) u if f > 1/2: the chain is an INTEGER prefix sum of D_i = A_i + [f_i > 1/2] - one wave scan.  Exactly two things
// break that, and both are rare: f_i = 1/2 exactly (round-half-even: the result depends on the parity of M - A), and a result that
// leaves the binade (the grid gets finer).  The scan is taken up to the first such lane (the prefix test M - P >= 2^52 + 1 keeps
// every bulk step's exact difference inside the binade: its rounding moves it by at most u/2), that one lane is subtracted by the
// hardware, and the rest goes round again in whatever binade the value is in then.  Lanes with x == 0 change nothing (r - 0 == r).
// Anything that is not a positive normal number - r <= 0, a negative, subnormal or non-finite x - takes the plain chain.
// Wave-uniform in r, per-lane in x; every lane returns the result.  Checked against the plain chain on adversarial inputs (exact
// halves, binade exits, zeros, x >= r) by tests/test_gpu_parity.py::test_float_chain_by_integer_scan.
__device__ __forceinline__ double chain_subtract_wave(double r, double x)
{
    const int lane = (int)(threadIdx.x & 63u);
    unsigned long long todo = __builtin_amdgcn_ballot_w64(x != 0.0);
    const unsigned long long sb = (unsigned long long)__double_as_longlong(x);
    const int e_s = (int)((sb >> 52) & 0x7FFull);
    const unsigned long long m_s = (sb & 0x000FFFFFFFFFFFFFull) | 0x0010000000000000ull;
    const bool x_plain = (sb >> 63) == 0ull && e_s != 0 && e_s != 2047;          // a positive normal number
    while (todo) {
        const unsigned long long rb = (unsigned long long)__double_as_longlong(r);
        const int e_r = (int)(rb >> 52);                                         // (sign bit clear below)
        if (!(r > 0.0) || e_r == 0 || e_r >= 2047) {
            while (todo) {                                                        // the plain chain for what is left
                const int l = __ffsll((long long)todo) - 1;
                todo &= todo - 1ull;
                r -= readlane_f64(x, l);
            }
            break;
        }
        const long long M = (long long)((rb & 0x000FFFFFFFFFFFFFull) | 0x0010000000000000ull);
        const bool in = (todo >> lane) & 1ull;
        const int k = e_r - e_s;                                                  // x = m_s 2^-k in units of u
        long long D = 0;
        bool special = false;
        if (in) {
            if (!x_plain || k < 1) special = true;                                // (k < 1: x is at least 2^E: the difference leaves the binade)
            else if (k <= 53) {
                const unsigned long long rem = m_s & ((1ull << k) - 1ull), half = 1ull << (k - 1);
                D = (long long)(m_s >> k) + (rem > half ? 1ll : 0ll);
                special = rem == half;                                            // round-half-even: by the hardware
            }                                                                     // (k >= 54: x < u / 2, the difference rounds back to r)
        }
        const long long P = wave_scan_i64(D);                                     // inclusive prefix of the decrements
        const bool bad = in && (special || M - P < (1ll << 52) + 1ll);
        const unsigned long long bm = __builtin_amdgcn_ballot_w64(bad);
        const int l = bm ? __ffsll((long long)bm) - 1 : kWave;
        const long long pre = l == 0 ? 0ll : readlane_i64(P, l - 1);             // what the lanes before l take together
        r = __longlong_as_double((long long)(((unsigned long long)e_r << 52) | ((unsigned long long)(M - pre) & 0x000FFFFFFFFFFFFFull)));
        if (l < kWave) {
            r -= readlane_f64(x, l);
            todo &= ~((2ull << l) - 1ull);
        } else todo = 0ull;
    }
    return r;
}

// acc += bit `lane` of mask: one v_addc_co_u32 with the mask as carry-in (hipcc otherwise materialises the bit with a
// VOP3 v_cndmask and adds it: two half-rate instructions)
__device__ __forceinline__ void add_lane_bit(unsigned int &acc, unsigned long long mask)
{
    unsigned long long carry_out;
    asm("v_addc_co_u32 %0, %1, 0, %0, %2" : "+v"(acc), "=s"(carry_out) : "s"(mask));
}

// log table of the auction law (adc_law.h neg_log_u24), one copy per device, filled at engine creation
__device__ adc::LogTableEntry g_log_table[adc::kLogTableIntervals];

// normal-quantile table (adc_law.h normal_tab): volume and revenue draws
__device__ adc::NormTableEntry g_norm_table[adc::kNormTableEntries];
__device__ float g_norm_nodes[adc::kNormTableEntries + 1];       // the node values alone (+ the p = 1/2 node), for LDS copies
__device__ float g_log_nodes[adc::kLogTableIntervals + 1];       // node values of g_log_table (+ log 2), for LDS copies (adc::LogNodes)

__global__ void k_build_log_table()
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < adc::kLogTableIntervals) g_log_table[i] = adc::log_table_entry(i);
    if (i < adc::kNormTableEntries) g_norm_table[i] = adc::norm_table_entry(i);
    if (i <= adc::kNormTableEntries) g_norm_nodes[i] = adc::norm_table_node(i);
    if (i <= adc::kLogTableIntervals) g_log_nodes[i] = adc::log_table_node(i);
}

// update_keywords() of one keyword given its three coefficients (adcraft/gymnasium_kw_env.py:136-158)
__device__ __forceinline__ void apply_drift_coefficients(float uv, float uc, float us, float &vol_mean, float vol_std, float &bctr,
                                                         float &sctr)
{
    const float nv = adc::fma32(uv, vol_std, vol_mean);            // "init volume" is the vol std (:136-137)
    vol_mean = nv > 0.0f ? nv : 0.0f;
    bctr = adc::clamp01(bctr * (1.0f + uc));
    sctr = adc::clamp01(sctr * (1.0f + us));
}

// View::drift_bits and View::drift_rate are read from the kernel-argument segment where they are used, inside the drift
// branch: every kernel with a drift site takes the engine view `v` as its first argument, at offset 0, so the helpers below
// must only be given that `v`.  (Read through `v`, the two pointers are loaded with the rest of the view at the kernel's entry
// and hold scalar registers through the whole kernel: the row kernels have none to spare and spill more - 4 to 12 bytes of
// scratch per lane more in k_step_exact_rows.)  kernel_sparse.inc re-reads its pointers the same way.
typedef const __attribute__((address_space(4))) View DriftArgView;
__device__ __forceinline__ DriftArgView *drift_args()
{
    DriftArgView *p = (DriftArgView *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

// does keyword k of env `env` (of the view) move at update_keywords()?  Every drift site asks this first, inside its drift
// branch: an unselected keyword keeps vol_mean, bctr and sctr as they are (its draw is simply not taken; nothing else moves)
__device__ __forceinline__ bool drift_selected(const View &v, int env, int k)
{
    const uint32_t *bits = drift_args()->drift_bits;
    if (!bits) return true;
    const unsigned int words = ((unsigned int)v.K + 31u) >> 5;       // (N * words < 2^31: N * K does)
    return ((bits[(unsigned int)env * words + ((unsigned int)k >> 5)] >> (k & 31)) & 1u) != 0u;
}

// the env's three drift magnitudes (View::drift_rate, or the engine's scalars)
__device__ __forceinline__ void drift_magnitudes(const View &v, int env, float &a_vol, float &a_ctr, float &a_cvr)
{
    const float *rate = drift_args()->drift_rate;
    if (rate) {
        const float *r = rate + (size_t)env * 3;
        a_vol = r[0]; a_ctr = r[1]; a_cvr = r[2];
    } else {
        a_vol = v.drift_vol; a_ctr = v.drift_ctr; a_cvr = v.drift_cvr;
    }
}

// pending drift of one keyword (adcraft/gymnasium_kw_env.py:132-158); `tick_of_draw` = tick of the
// step whose update_keywords() this is.  false: the keyword is not selected and nothing was changed (no write-back needed)
__device__ __forceinline__ bool drift_keyword(const View &v, int env, uint64_t key, uint32_t tick_of_draw, int k,
                                              float &vol_mean, float vol_std, float &bctr, float &sctr)
{
    if (!drift_selected(v, env, k)) return false;
    float a_vol, a_ctr, a_cvr;
    drift_magnitudes(v, env, a_vol, a_ctr, a_cvr);
    const adc::U4 w = adc::draw(key, 0u, adc::ST_DRIFT, (uint32_t)k, tick_of_draw);
    apply_drift_coefficients(adc::drift_coeff(w.x, a_vol), adc::drift_coeff(w.y, a_ctr), adc::drift_coeff(w.z, a_cvr),
                             vol_mean, vol_std, bctr, sctr);
    return true;
}

// ... read from the parameter planes and written back there (a selected keyword only)
__device__ __forceinline__ void drift_keyword_planes(const View &v, int env, uint64_t key, uint32_t tick_of_draw, int k)
{
    if (!drift_selected(v, env, k)) return;
    float vm = param_at(v, ADC_P_VOL_MEAN, env, k), bc = param_at(v, ADC_P_BCTR, env, k), sc = param_at(v, ADC_P_SCTR, env, k);
    drift_keyword(v, env, key, tick_of_draw, k, vm, param_at(v, ADC_P_VOL_STD, env, k), bc, sc);
    param_at(v, ADC_P_VOL_MEAN, env, k) = vm;
    param_at(v, ADC_P_BCTR, env, k) = bc;
    param_at(v, ADC_P_SCTR, env, k) = sc;
}
