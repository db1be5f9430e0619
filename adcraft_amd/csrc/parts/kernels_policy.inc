// kernels_policy.inc - the callers of the step, on the device: the paper's baseline bidder, the oracle bidder and the
// per-step ideal profit (the loop of baseline_experiment_and_figs_notebooks/run_heatmap_experiments.ipynb cell 1 and
// timing_and_other_one_off_experiments.ipynb cell 2).  (part of the single translation unit adc_engine.hip)
// -------------------------------------------------------------------------------------------------
// one line of a keyword's curve that can be the argmax, with the margin interval on which it can (k_curve_contenders)
struct ContenderEntry {
    float lo, hi;              // margins (sctr x rev_mean) for which this line is within reach of the envelope
    unsigned int x, y;         // the curve point itself (PolicyView::curve)
    unsigned int b, pad;       // its grid index
};

struct PolicyView {
    // NaiveZeroMarginStrategy caches (adcraft/baselines/interpolated_expectations.py:286-295, 442-515), [N][K]
    float *ave_rpc;
    int32_t *n_rpc;
    float *ave_sctr;
    int32_t *n_sctr;
    double *max_bid;
    uint64_t *key;             // [N] the agent's own stream
    uint32_t *tick;            // [N]
    float default_rpc;
    // bid curves of every keyword on the bid grid (get_implicit_kw_bid_cpc_impressions), [N*K][n_bids], 8 bytes per
    // point: x = numerator of the expected cpc in cents, y = (samples <= bid) | bit 31 if that is all of them
    uint2 *curve;
    int n_samples;
    double *grid;              // [n_bids]
    int n_bids;
    double *ideal;             // [N][K] last evaluation of get_max_expected_bid_profits
    int32_t *best;             // [N][K] its argmax over the grid
    double *sum_ideal;         // [N][K] running sum of ideal            (compute_NCP's denominator)
    double *sum_ideal_pos;     // [N][K] running sum of ideal, <= 0 -> 1 (compute_AKNCP's denominator, :71-75)
    // contenders of every keyword's curve (k_curve_contenders): its distinct grid points that come within reach of the upper
    // envelope, ascending, each with the margin interval [x, y] on which it does; [N*K][cont_cap] + their number
    // (kContenderAll: evaluate the whole grid) + where the last search ended
    ContenderEntry *contender;
    uint16_t *n_contenders;
    uint16_t *cont_pos;
    int cont_cap;
    // EXPLICIT keywords (k_explicit_curves): instead of `curve`, per keyword {z_lo, z_hi, impression intercept, impression slope}
    // (16 bytes, [N*K]) and per grid point the cost law's mu_b, sigma_b ([n_bids]); every point is recomputed from them
    float4 *xcurve;
    double *grid_mu, *grid_sigma;
};
constexpr unsigned short kContenderAll = 0xFFFFu;
constexpr double kMarginMax = 1.0e6;          // margins (sctr x rev_mean, dollars) beyond this evaluate the whole grid

// 53-bit uniform in [0,1) from two words, as numpy's Generator.random() makes one from 64 bits
__device__ __forceinline__ double uniform53(uint32_t a, uint32_t b)
{
    return (double)(((unsigned long long)(a >> 5) << 26) | (unsigned long long)(b >> 6)) * 1.1102230246251565e-16;
}

// NaiveZeroMarginStrategy.update_all_caches (:485-494) for one observation per keyword, then sample_action
// (:496-515).  torch.Tensor(observation) is float32, so the cache arithmetic is float32 (one correctly rounded op
// each, in the reference's order); the bid is a float64 product of the float32 cache values.
// One workgroup per env; lanes stride over keywords; the budget is 100 x the sum of the per-keyword branch codes.
__global__ __launch_bounds__(256) void k_agent_step(View v, PolicyView p, const int32_t *__restrict__ clicks,
                                                    const int32_t *__restrict__ convs, const float *__restrict__ revenue,
                                                    int do_update, int do_act, const double *__restrict__ replay_u,
                                                    float budget_override, float *__restrict__ bids, float *__restrict__ budgets)
{
    __shared__ int part[256 / kWave];
    const int env = blockIdx.x, K = v.K;
    const uint64_t key = p.key[env];
    const uint32_t tick = p.tick[env];
    int code_sum = 0;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const size_t o = (size_t)env * K + k;
        float ave_rpc = p.ave_rpc[o], ave_sctr = p.ave_sctr[o];
        int n_rpc = p.n_rpc[o], n_sctr = p.n_sctr[o];
        if (do_update) {
            const float bc = (float)clicks[o], sc = (float)convs[o], rev = revenue[o];
            if (bc > 0.0f) {                                                   // :116-117
                if (sc > 0.0f) {                                               // :127-128: a revenue observation
                    const float rpc_obs = rev / sc;                            // :130
                    const float term = (float)((double)ave_rpc * (double)n_rpc);          // python float * int, cast into the f32 sum
                    ave_rpc = (rpc_obs + term) / (float)(n_rpc + 1);           // :75-77
                    n_rpc += 1;                                                // :78
                }
                const float s_obs = sc / bc;                                   // :121-123
                const float termc = (float)((double)ave_sctr * (double)n_sctr);
                const float all_convs = s_obs * bc + termc;                    // :97 (bc = float(clicks))
                const double all_obs = (double)clicks[o] + (double)n_sctr;     // :96
                ave_sctr = all_convs / (float)(all_obs > 1.0 ? all_obs : 1.0); // :99
                n_sctr += 1;                                                   // :101
            }
            p.ave_rpc[o] = ave_rpc;
            p.n_rpc[o] = n_rpc;
            p.ave_sctr[o] = ave_sctr;
            p.n_sctr[o] = n_sctr;
        }
        if (do_act) {
            double bid;
            int code;
            if (n_rpc < 1) {
                double u;
                if (replay_u) u = replay_u[o];
                else {
                    const adc::U4 w = adc::draw(key, 0u, adc::ST_AGENT, (uint32_t)k, tick);
                    u = uniform53(w.x, w.y);
                }
                // rng.random() <= 1 / np.sqrt(num_sctr_obs)  (:501; 1/sqrt(0) = inf: always)
                const bool ramp = n_sctr == 0 || u <= 1.0 / __builtin_sqrt((double)n_sctr);
                if (ramp) {
                    double nb = p.max_bid[o] + 0.03;                           // :503
                    nb = nb < 3.0 ? nb : 3.0;
                    nb = nb > 0.01 ? nb : 0.01;
                    p.max_bid[o] = nb;
                    bid = nb;
                    code = 1;
                } else {
                    bid = (double)ave_sctr * (double)p.default_rpc;            // :507
                    code = 2;
                }
            } else {
                bid = (double)ave_rpc * (double)ave_sctr;                      // :510-511 via :196-199
                code = 3;
            }
            // the env rounds the float64 bid to cents (gymnasium_kw_env.py:215); hand over exactly that value
            double c = __builtin_rint(bid * 100.0);
            c = c >= 1.0 ? c : 1.0;
            c = c < 1.0e9 ? c : 1.0e9;
            bids[o] = (float)(c / 100.0);
            code_sum += code;
        }
    }
    if (!do_act) return;
    code_sum = (int)wave_sum_i64(code_sum);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = code_sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int i = 0; i < (int)(blockDim.x / kWave); ++i) t += part[i];
        budgets[env] = budget_override > 0.0f ? budget_override : 100.0f * (float)t;       // :515
        p.tick[env] = tick + 1u;
    }
}

struct CurveLine { double s, c; };          // slope = impression rate, zero crossing = cpc
// an EXPLICIT keyword's cached curve: every kernel reads its points through at(), i.e. adc::explicit_curve_point
struct ExplicitCurve {
    float thresh, a, b, z_lo, z_hi;
    const double *grid, *mu, *sigma;
    __device__ __forceinline__ CurveLine at(int bi) const
    {
        const adc::CurvePoint q = adc::explicit_curve_point(thresh, a, b, z_lo, z_hi, grid[bi], mu[bi], sigma[bi]);
        return CurveLine{q.ir, q.cpc};
    }
};
__device__ __forceinline__ ExplicitCurve explicit_curve(const View &v, const PolicyView &p, size_t o)
{
    const float4 c = p.xcurve[o];
    return ExplicitCurve{v.imp_thresh, c.z, c.w, c.x, c.y, p.grid, p.grid_mu, p.grid_sigma};
}

// get_max_expected_bid_profits (experiment_metrics.py:40-61) for the CURRENT parameters against the cached curves:
// profit(b) = max(vol_mean * IR(b) * bctr * (sctr * rev_mean - cpc(b)), 0); ideal = max(0, max_b), best = argmax_b
// (first index of the maximum, as np.argmax).  One wavefront per keyword.
template <int MODEL>
__global__ __launch_bounds__(256) void k_ideal_from_curves(View v, PolicyView p, int accumulate)
{
    const int lane = threadIdx.x & 63;
    const size_t o = (size_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x >> 6);
    if (o >= (size_t)v.N * v.K) return;                    // (whole wavefronts leave together)
    const int env = (int)(o / v.K), k = (int)(o - (size_t)env * v.K);
    const double vol_mean = param_at(v, ADC_P_VOL_MEAN, env, k), bctr = param_at(v, ADC_P_BCTR, env, k);
    const double margin = (double)param_at(v, ADC_P_SCTR, env, k) * (double)param_at(v, ADC_P_REV_MEAN, env, k);
    double best = -1.0;
    int best_i = 0x7FFFFFFF;
    if constexpr (MODEL == ADC_MODEL_EXPLICIT) {
        const ExplicitCurve cv = explicit_curve(v, p, o);
        for (int bi = lane; bi < p.n_bids; bi += kWave) {
            const CurveLine l = cv.at(bi);
            double pr = vol_mean * l.s * bctr * (margin - l.c);
            pr = pr > 0.0 ? pr : 0.0;
            if (pr > best) { best = pr; best_i = bi; }
        }
    } else {
    const uint2 *curve = p.curve + o * p.n_bids;
    const double n_samples = (double)p.n_samples;
    // idx / n: a power-of-two n (the notebooks' 2048) divides exactly by multiplying with its reciprocal
    const bool pow2 = (p.n_samples & (p.n_samples - 1)) == 0;
    const double inv_n = 1.0 / n_samples;
    // HBM-bound stream of 8 bytes per grid point: every lane issues all the loads of a 320-point chunk before it
    // computes (5 x 512 B per wavefront in flight; one load at a time reached 2.9 TB/s)
    constexpr int kPer = 5;
    for (int base = 0; base < p.n_bids; base += kPer * kWave) {
        uint2 c[kPer];
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int bi = base + i * kWave + lane;
            c[i] = bi < p.n_bids ? curve[bi] : make_uint2(0u, 0u);
        }
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int bi = base + i * kWave + lane;
            if (bi >= p.n_bids) continue;
            const unsigned int idx = c[i].y & 0x7FFFFFFFu;
            const double ir = pow2 ? (double)idx * inv_n : (double)idx / n_samples;             // experiment_metrics.py:32
            const double dollars = c[i].x < 0x80000000u ? adc::cents_to_dollars_f64((int)c[i].x) : (double)c[i].x / 100.0;
            const double cpc = dollars / ((c[i].y >> 31) ? n_samples : (double)(idx + 1u));     // :33-35
            double pr = vol_mean * ir * bctr * (margin - cpc);
            pr = pr > 0.0 ? pr : 0.0;
            if (pr > best) { best = pr; best_i = bi; }      // a lane's indices ascend: keeps its first maximum
        }
    }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const double ob = __shfl_xor(best, s, 64);
        const int oi = __shfl_xor(best_i, s, 64);
        if (ob > best || (ob == best && oi < best_i)) { best = ob; best_i = oi; }
    }
    if (lane == 0) {
        const double ideal = best > 0.0 ? best : 0.0;
        p.ideal[o] = ideal;
        p.best[o] = best_i;
        if (accumulate) {
            p.sum_ideal[o] += ideal;
            p.sum_ideal_pos[o] += ideal <= 0.0 ? 1.0 : ideal;
        }
    }
}

// ---- the per-step ideal in a fraction of the grid ------------------------------------------------------------------------
// profit_b(m) = (vol_mean bctr) ir_b (m - cpc_b) with m = sctr rev_mean: for a keyword, 299 LINES in the one scalar that drifts.
// The argmax over the grid depends on m alone; as m grows it moves up the grid along the lines' upper envelope - so nearly every
// distinct grid point is the argmax for SOME m, but for a GIVEN m only the envelope's active line and what lies within rounding
// distance of it.  k_curve_contenders finds, once per curve build, for every distinct line the m-interval on which it comes
// within reach of the envelope; k_ideal_from_contenders then looks up the few lines whose interval holds today's m (a
// bracketing search that starts where yesterday's ended) and evaluates the EXACT float64 expression of the full scan on them,
// keeping the first maximum, as np.argmax does.
//
// Why the result is the full scan's, bit for bit: the scan returns the first index whose ROUNDED profit is maximal.  Every
// rounded profit is within 4 ulp (relative 4.5e-16: one exactly rounded subtraction of two exact inputs, three products) of its
// real value, so the winner's real value is within 1e-15 (relative) of the envelope's at m.  A line's interval is where
// f_b(m) >= (1 - kRel) env(m) - kAbs with kRel = 1e-9, kAbs = 1e-12 - a million times that distance (it also absorbs the
// rounding of this analysis itself, done in float64) - widened to whole envelope segments, stored as float32 rounded outwards,
// and made monotone along the list (prefix maximum of the upper ends, suffix minimum of the lower ones), so that the lines
// whose interval holds m are one contiguous run of the list.  f_b - (1 - kRel) env is concave in m: it is >= -kAbs on an
// interval around the envelope breakpoint where the envelope's slope passes the line's.  Identical lines (runs of grid points
// between two sampled competitor bids: same count, same sum) can only be won by their FIRST point (strict comparison): the
// later ones are dropped.  No positive profit -> index 0, as the scan's.  A margin outside [0, kMarginMax] (or not finite), or a
// curve with more distinct lines than the lists hold -> the whole grid.

__device__ __forceinline__ CurveLine curve_line(uint2 pt, double n_samples, double inv_n, bool pow2)
{
    const unsigned int idx = pt.y & 0x7FFFFFFFu;
    CurveLine l;
    l.s = pow2 ? (double)idx * inv_n : (double)idx / n_samples;                                   // as k_ideal_from_curves
    const double dollars = pt.x < 0x80000000u ? adc::cents_to_dollars_f64((int)pt.x) : (double)pt.x / 100.0;
    l.c = dollars / ((pt.y >> 31) ? n_samples : (double)(idx + 1u));
    return l;
}
__device__ __forceinline__ float float_below(double x)
{
    float f = (float)x;
    if ((double)f > x) f = __uint_as_float(f > 0.0f ? __float_as_uint(f) - 1u : f < 0.0f ? __float_as_uint(f) + 1u : 0x80000001u);
    return f;
}
__device__ __forceinline__ float float_above(double x)
{
    float f = (float)x;
    if ((double)f < x) f = __uint_as_float(f > 0.0f ? __float_as_uint(f) + 1u : f < 0.0f ? __float_as_uint(f) - 1u : 0x00000001u);
    return f;
}

// One WAVEFRONT per keyword.  LDS per wave: the distinct lines (slope, zero crossing, grid index) and their intervals.  Every pass is
// wave-parallel (round 5; until then lane 0 ran the hull as a serial stack - 71 000 of the kernel's 103 000 cycles per keyword at cfg2, ~820
// per line of branchy scalar-lane code - and walked the kept list twice):
//   * the upper envelope by ELIMINATION IN PLACE: every line tests itself against its two neighbours in the list (the monotone chain's own
//     test: t is never the maximum if the line after it overtakes the line before it no later than t does), the survivors are compacted to
//     the front of the arrays, and that repeats until a pass removes nothing.  A line that fails the test against ANY pair of lines is
//     nowhere strictly above both, so lines removed together - neighbours included - are all off the envelope; a list whose every
//     consecutive triple passes is the envelope (slopes ascend).  The notebooks' curves keep ~95 % of their ~90 distinct lines: two or
//     three passes.  Each lane holds its own lines in registers for the interval pass, whose slots the compaction reuses;
//   * the monotone ends of the kept list by wave scans.
// n_bids <= kContenderLines.
constexpr int kContenderLines = 304;          // (the notebooks' grid has 299 points; 304 lines = 8516 bytes: seven of gfx950's 1280-byte LDS blocks, 18 wavefronts per CU - 320 took eight: 16)
constexpr int kContenderChunks = (kContenderLines + kWave - 1) / kWave;
struct ContenderScratch {
    double s[kContenderLines], c[kContenderLines];      // the lines in grid order; after the envelope pass: [0, n_hull) the envelope, lowest slope first
    float lo[kContenderLines], hi[kContenderLines];
    unsigned short b[kContenderLines];
    unsigned short keep[kContenderLines];
};
static_assert(sizeof(ContenderScratch) <= 7 * 1280, "k_curve_contenders: seven LDS blocks per wavefront");

template <int MODEL>
__global__ __launch_bounds__(kWave) void k_curve_contenders(View v, PolicyView p)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    ContenderScratch &w = *reinterpret_cast<ContenderScratch *>(lds_raw);
    const int lane = threadIdx.x;
    const size_t o = blockIdx.x;
    constexpr double kRel = 1.0e-9, kAbs = 1.0e-12;
    const unsigned long long lt = lanemask_lt();

    int n_lines = 0;
    if constexpr (MODEL == ADC_MODEL_EXPLICIT) {
        // the distinct lines with a positive slope, in grid order.  The elimination below needs ascending slopes: a curve whose impression
        // rate ever falls along the grid (a negative slope parameter, an unsorted grid, rounding) is evaluated on the whole grid
        const ExplicitCurve cv = explicit_curve(v, p, o);
        CurveLine ls[kContenderChunks];
#pragma unroll
        for (int ch = 0; ch < kContenderChunks; ++ch) {
            const int b = ch * kWave + lane;
            ls[ch] = b < p.n_bids ? cv.at(b) : CurveLine{0.0, 0.0};
        }
        bool falls = false;
        double carry_s = 0.0, carry_c = 0.0;            // the previous chunk's last line
#pragma unroll
        for (int ch = 0; ch < kContenderChunks; ++ch) {
            const int b = ch * kWave + lane;
            if (ch * kWave >= p.n_bids) break;                  // (wave-uniform)
            double ps = __shfl_up(ls[ch].s, 1, kWave), pc = __shfl_up(ls[ch].c, 1, kWave);
            if (lane == 0) { ps = carry_s; pc = carry_c; }
            carry_s = __shfl(ls[ch].s, kWave - 1, kWave);
            carry_c = __shfl(ls[ch].c, kWave - 1, kWave);
            const CurveLine l = ls[ch];
            bool keep = false;
            if (b < p.n_bids) {
                falls |= b > 0 && !(l.s >= ps);
                keep = !(b > 0 && l.s == ps && l.c == pc) && l.s > 0.0 && l.c == l.c;
            }
            const unsigned long long m = __ballot(keep);
            if (keep) {
                const int at = n_lines + (int)__popcll(m & lt);
                w.s[at] = l.s; w.c[at] = l.c; w.b[at] = (unsigned short)b;
            }
            n_lines += (int)__popcll(m);
        }
        if (__ballot(falls)) {
            if (lane == 0) { p.cont_pos[o] = 0; p.n_contenders[o] = kContenderAll; }
            return;
        }
    } else {
    const uint2 *curve = p.curve + o * p.n_bids;
    const double n_samples = (double)p.n_samples, inv_n = 1.0 / n_samples;
    const bool pow2 = (p.n_samples & (p.n_samples - 1)) == 0;

    // the distinct lines with a positive slope, in grid order.  All of the curve's points are requested before the first is used (the
    // compaction below carries a count from chunk to chunk: chunk by chunk the loads would be five HBM round trips in a row).  The
    // elimination below needs ascending slopes: a point's idx never falls along an ascending grid - a curve where it does (a descending or
    // shuffled grid) is evaluated on the whole grid, as the EXPLICIT instance does
    uint2 pts[kContenderChunks], pvs[kContenderChunks];
#pragma unroll
    for (int ch = 0; ch < kContenderChunks; ++ch) {
        const int b = ch * kWave + lane;
        pts[ch] = b < p.n_bids ? curve[b] : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        pvs[ch] = b > 0 && b < p.n_bids ? curve[b - 1] : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
    }
    bool falls = false;
#pragma unroll
    for (int ch = 0; ch < kContenderChunks; ++ch) {
        const int b = ch * kWave + lane;
        if (ch * kWave >= p.n_bids) break;                      // (wave-uniform)
        bool keep = false;
        CurveLine l{0.0, 0.0};
        if (b < p.n_bids) {
            const uint2 pt = pts[ch], pv = pvs[ch];
            l = curve_line(pt, n_samples, inv_n, pow2);
            keep = !(pt.x == pv.x && pt.y == pv.y) && l.s > 0.0 && l.c == l.c;
            falls |= b > 0 && (pt.y & 0x7FFFFFFFu) < (pv.y & 0x7FFFFFFFu);
        }
        const unsigned long long m = __ballot(keep);
        if (keep) {
            const int at = n_lines + (int)__popcll(m & lt);
            w.s[at] = l.s; w.c[at] = l.c; w.b[at] = (unsigned short)b;
        }
        n_lines += (int)__popcll(m);
    }
    if (__ballot(falls)) {
        if (lane == 0) { p.cont_pos[o] = 0; p.n_contenders[o] = kContenderAll; }
        return;
    }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    unsigned short *out_n = p.n_contenders + o;
    if (lane == 0) p.cont_pos[o] = 0;
    if (n_lines == 0) { if (lane == 0) *out_n = 0; return; }        // no line is ever positive: index 0, ideal 0

    // this lane's own lines, for the interval pass (the envelope pass compacts the arrays in place)
    double own_s[kContenderChunks], own_c[kContenderChunks];
#pragma unroll
    for (int ch = 0; ch < kContenderChunks; ++ch) {
        const int i = ch * kWave + lane;
        own_s[ch] = i < n_lines ? w.s[i] : 0.0;
        own_c[ch] = i < n_lines ? w.c[i] : 0.0;
    }
    // upper envelope by elimination in place (see above).  Chunk by chunk in list order: a chunk reads its lines and their neighbours, then
    // writes its survivors at or below their own positions - never over a line that a later chunk still reads, except with itself
    int size = n_lines;
    for (;;) {
        int kept = 0;
        for (int base = 0; base < size; base += kWave) {
            const int i = base + lane;
            bool keep = false;
            double ls = 0.0, lc = 0.0;
            if (i < size) {
                ls = w.s[i]; lc = w.c[i];
                keep = true;
                if (i > 0) {
                    const double us = w.s[i - 1], uc = w.c[i - 1];
                    if (us == ls) keep = lc < uc;                           // parallel: the one that crosses zero first is above everywhere (a tie keeps the earlier)
                    else if (i + 1 < size) {
                        const double rs = w.s[i + 1], rc = w.c[i + 1];
                        // never the maximum if r overtakes u no later than this line does: x(u,r) <= x(u,l), denominators > 0
                        const double iu = us * uc, il = ls * lc, ir = rs * rc;
                        if (rs != ls && (ir - iu) * (ls - us) <= (il - iu) * (rs - us)) keep = false;
                    }
                }
                if (keep && i + 1 < size) { const double rs = w.s[i + 1], rc = w.c[i + 1]; if (rs == ls && rc < lc) keep = false; }
            }
            const unsigned long long m = __ballot(keep);
            if (keep) { const int at = kept + (int)__popcll(m & lt); w.s[at] = ls; w.c[at] = lc; }
            kept += (int)__popcll(m);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        if (kept == size) break;
        size = kept;
    }
    auto hs = [&](int j) { return w.s[j]; };
    auto breakpoint = [&](int j) -> double {       // where hull line j + 1 overtakes hull line j (j = -1: -inf, j = size - 1: +inf)
        if (j < 0) return -__builtin_inf();
        if (j + 1 >= size) return __builtin_inf();
        const int qa = j, qb = j + 1;
        return (w.s[qb] * w.c[qb] - w.s[qa] * w.c[qa]) / (w.s[qb] - w.s[qa]);
    };
    // per line: the margin interval on which it is within reach of the envelope (whole envelope segments)
#pragma unroll
    for (int ch = 0; ch < kContenderChunks; ++ch) {
        const int i = ch * kWave + lane;
        if (i >= n_lines) continue;
        const double ls = own_s[ch], lc = own_c[ch];
        int lo = 0, hi = size - 1;
        while (lo < hi) {                                       // first hull line whose relaxed slope reaches this line's
            const int mid = (lo + hi) >> 1;
            if ((1.0 - kRel) * hs(mid) < ls) lo = mid + 1; else hi = mid;
        }
        auto gap_at = [&](int j) {                              // at breakpoint j, clamped to finite margins
            double m = breakpoint(j);
            m = m < -kMarginMax ? -kMarginMax : m > kMarginMax ? kMarginMax : m;
            const int qa = j < 0 ? 0 : j, qb = j + 1 >= size ? size - 1 : j + 1;
            const double e1 = w.s[qa] * (m - w.c[qa]), e2 = w.s[qb] * (m - w.c[qb]), envl = e1 > e2 ? e1 : e2;
            return ls * (m - lc) - (1.0 - kRel) * envl + kAbs;
        };
        // the concave gap peaks at breakpoint lo - 1 (hull line lo takes over there); the slopes' own rounding may move it by one
        int jl = lo - 1;
        bool reach = gap_at(jl) >= 0.0;
        if (!reach && gap_at(lo) >= 0.0) { jl = lo; reach = true; }
        if (!reach && lo >= 2 && gap_at(lo - 2) >= 0.0) { jl = lo - 2; reach = true; }
        float f_lo = __builtin_inff(), f_hi = -__builtin_inff();        // (an empty interval: can never be the argmax)
        if (reach) {
            int jr = jl;
            while (jl >= 0 && gap_at(jl - 1) >= 0.0) --jl;      // widen while the neighbouring breakpoints are within reach too
            while (jr + 1 < size && gap_at(jr + 1) >= 0.0) ++jr;
            f_lo = float_below(breakpoint(jl - 1));             // whole segments beyond the outermost breakpoints within reach
            f_hi = float_above(breakpoint(jr + 1));
        }
        w.lo[i] = f_lo; w.hi[i] = f_hi;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // compact the lines that have an interval; make the ends monotone along the list (prefix max of the upper ends, suffix min
    // of the lower ones): the lines whose interval holds a given margin are then one contiguous run
    int n_out = 0;
    for (int base = 0; base < n_lines; base += kWave) {
        const int i = base + lane;
        const bool keep = i < n_lines && w.lo[i] <= w.hi[i];
        const unsigned long long m = __ballot(keep);
        if (keep) w.keep[n_out + (int)__popcll(m & lt)] = (unsigned short)i;
        n_out += (int)__popcll(m);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (n_out > p.cont_cap) { if (lane == 0) *out_n = kContenderAll; return; }
    // (64 list entries at a time by a wave scan - max and min of floats that are never NaN: the kept intervals satisfy lo <= hi - carried
    //  from chunk to chunk)
    {
        float carry = -__builtin_inff();
        for (int base = 0; base < n_out; base += kWave) {
            const int r = base + lane;
            const int i = r < n_out ? (int)w.keep[r] : 0;
            float x = r < n_out ? w.hi[i] : -__builtin_inff();
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) { const float y = __shfl_up(x, d, kWave); if (lane >= d) x = y > x ? y : x; }
            x = carry > x ? carry : x;
            if (r < n_out) w.hi[i] = x;
            carry = __shfl(x, kWave - 1, kWave);
        }
        carry = __builtin_inff();
        for (int base = ((n_out - 1) / kWave) * kWave; base >= 0; base -= kWave) {
            const int r = base + lane;
            const int i = r < n_out ? (int)w.keep[r] : 0;
            float x = r < n_out ? w.lo[i] : __builtin_inff();
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) { const float y = __shfl_down(x, d, kWave); if (lane + d < kWave) x = y < x ? y : x; }
            x = carry < x ? carry : x;
            if (r < n_out) w.lo[i] = x;
            carry = __shfl(x, 0, kWave);
        }
        if (lane == 0) *out_n = (unsigned short)n_out;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    ContenderEntry *out = p.contender + o * p.cont_cap;
    for (int r = lane; r < n_out; r += kWave) {
        const int i = w.keep[r];
        uint2 pt = make_uint2(0u, 0u);                          // (EXPLICIT: the point is recomputed from its grid index)
        if constexpr (MODEL == ADC_MODEL_IMPLICIT) pt = p.curve[o * p.n_bids + w.b[i]];
        out[r] = ContenderEntry{w.lo[i], w.hi[i], pt.x, pt.y, (unsigned int)w.b[i], 0u};
    }
}

// get_max_expected_bid_profits on the lines within reach of the envelope at today's margin: one LANE per keyword
template <int MODEL>
__global__ __launch_bounds__(256) void k_ideal_from_contenders(View v, PolicyView p, int accumulate)
{
    const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= (size_t)v.N * v.K) return;
    const int env = (int)(o / v.K), k = (int)(o - (size_t)env * v.K);
    const double vol_mean = param_at(v, ADC_P_VOL_MEAN, env, k), bctr = param_at(v, ADC_P_BCTR, env, k);
    const double margin = (double)param_at(v, ADC_P_SCTR, env, k) * (double)param_at(v, ADC_P_REV_MEAN, env, k);
    const double n_samples = (double)p.n_samples, inv_n = 1.0 / n_samples;
    const bool pow2 = (p.n_samples & (p.n_samples - 1)) == 0;
    const int count = p.n_contenders[o];
    double best = -1.0;
    int best_i = 0x7FFFFFFF;
    ExplicitCurve cv{};
    if constexpr (MODEL == ADC_MODEL_EXPLICIT) cv = explicit_curve(v, p, o);
    auto eval = [&](uint2 pt, int bi) {
        CurveLine l;
        if constexpr (MODEL == ADC_MODEL_EXPLICIT) l = cv.at(bi);          // (EXPLICIT entries carry no point: recomputed from bi)
        else l = curve_line(pt, n_samples, inv_n, pow2);
        double pr = vol_mean * l.s * bctr * (margin - l.c);          // the operation order of k_ideal_from_curves / the reference
        pr = pr > 0.0 ? pr : 0.0;
        if (pr > best) { best = pr; best_i = bi; }                   // ascending indices: keeps the first maximum
    };
    const uint2 *curve = p.curve + o * p.n_bids;
    // (the error analysis behind the lists needs a finite, normal common factor: anything else - NaN, infinite, negative,
    // or so small that profits underflow - takes the whole grid, like a margin outside the lists' range)
    const double scale = vol_mean * bctr;
    const bool plain = scale == 0.0 || (scale >= 1.0e-200 && scale <= 1.0e200);
    if (count == kContenderAll || !plain || !(margin >= 0.0 && margin <= kMarginMax)) {
        for (int bi = 0; bi < p.n_bids; ++bi) {
            if constexpr (MODEL == ADC_MODEL_EXPLICIT) eval(make_uint2(0u, 0u), bi);
            else eval(curve[bi], bi);
        }
    } else {
        // (the scan's answer when nothing is positive is index 0 with profit 0: any point's clamped profit is >= 0, and a point
        // with no impressions has exactly 0 - no need to read grid point 0 itself)
        best = 0.0;
        best_i = 0;
        if (count > 0) {
            const ContenderEntry *list = p.contender + o * p.cont_cap;
            // bracket today's margin, starting where yesterday's search ended (the margin drifts by a few percent a day)
            const int pos_was = p.cont_pos[o];
            int pos = pos_was < count ? pos_was : count - 1;
            // yesterday's entry and its two neighbours are requested together: the margin moves by a few percent a day, so the walks below
            // nearly always end inside these three and run on registers - one round trip to the lists instead of five or six in a row
            const int p0 = pos;
            const ContenderEntry e0 = list[p0];
            const ContenderEntry em = p0 > 0 ? list[p0 - 1] : e0, ep = p0 + 1 < count ? list[p0 + 1] : e0;
            auto at = [&](int i) -> ContenderEntry { return i == p0 ? e0 : i == p0 - 1 ? em : i == p0 + 1 ? ep : list[i]; };
            while (pos + 1 < count && (double)at(pos).hi < margin) ++pos;
            while (pos > 0 && (double)at(pos).lo > margin) --pos;
            if (pos != pos_was) p.cont_pos[o] = (unsigned short)pos;
            int lo = pos, hi = pos;
            while (lo > 0 && (double)at(lo - 1).hi >= margin) --lo;
            while (hi + 1 < count && (double)at(hi + 1).lo <= margin) ++hi;
            for (int i = lo; i <= hi; ++i) {
                const ContenderEntry en = at(i);
                if ((double)en.lo <= margin && margin <= (double)en.hi) eval(make_uint2(en.x, en.y), (int)en.b);
            }
        }
    }
    const double ideal = best > 0.0 ? best : 0.0;
    p.ideal[o] = ideal;
    p.best[o] = best_i;
    if (accumulate) {
        p.sum_ideal[o] += ideal;
        p.sum_ideal_pos[o] += ideal <= 0.0 ? 1.0 : ideal;
    }
}

// run_oracle_agent (timing_and_other_one_off_experiments.ipynb cell 2): bid the grid point of maximum expected profit
__global__ void k_policy_oracle(View v, PolicyView p, float budget, float *__restrict__ bids, float *__restrict__ budgets)
{
    const int env = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < v.K) {
        const size_t o = (size_t)env * v.K + k;
        double c = __builtin_rint(p.grid[p.best[o]] * 100.0);
        c = c >= 1.0 ? c : 1.0;
        bids[o] = (float)(c / 100.0);
    }
    if (k == 0) budgets[env] = budget;
}

__global__ void k_agent_init(View v, PolicyView p, const uint64_t *seeds, uint64_t seed, int64_t env_id_base)
{
    const int env = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < v.K) {
        const size_t o = (size_t)env * v.K + k;
        p.ave_rpc[o] = 0.0f;           // get_empty_cache, :286-295
        p.n_rpc[o] = 0;
        p.ave_sctr[o] = 0.4f;
        p.n_sctr[o] = 0;
        p.max_bid[o] = 0.01;           // :481
    }
    if (k == 0) {
        p.key[env] = seeds ? splitmix64(seeds[env] ^ 0xA6E27B1D5C3F9E01ull)
                           : splitmix64(seed ^ splitmix64((uint64_t)(env_id_base + env) + 0x2545F4914F6CDD1Dull));
        p.tick[env] = 0u;
    }
}

// compute_AKNCP / compute_NCP of every env on the device (experiment_metrics.py:64-83): ratio_k = (profit_k / n) / (ideal_pos_k / n)
// in the host's operation order, its median over the keywords by a bitonic sort in LDS (numpy's median: the middle element,
// or the mean of the two middle ones), and NCP = sum profit / (sum ideal, or 1 if that is not positive).  One workgroup per env;
// 2 N doubles go to the host instead of 3 N K.  LDS: next_pow2(K) doubles (K <= 4096 -> 32 KB).
constexpr int kMedianBlock = 256;
constexpr int kMedianMaxK = 4096;

__global__ __launch_bounds__(kMedianBlock) void k_akncp_ncp(View v, PolicyView pol, double days, double *akncp, double *ncp)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    double *r = reinterpret_cast<double *>(lds_raw);
    __shared__ double s_den[kMedianBlock / kWave];
    __shared__ long long s_num[kMedianBlock / kWave];
    const int env = blockIdx.x, K = v.K, tid = threadIdx.x;
    int P = 1;
    while (P < K) P <<= 1;
    long long num = 0;
    double den = 0.0;
    int saw_nan = 0;                                 // np.median of a vector holding a NaN is NaN (closed_loop.py:38)
    for (int k = tid; k < P; k += kMedianBlock) {
        double x = __builtin_inf();                  // padding sorts to the top
        if (k < K) {
            const size_t o = (size_t)env * K + k;
            const long long pc = metric_total(v, o);
            x = ((double)pc / 100.0 / days) / (pol.sum_ideal_pos[o] / days);
            if (x != x) { x = __builtin_inf(); saw_nan = 1; }       // (a NaN ratio must not break the sort; the env's median is NaN below)
            num += pc;
            den += pol.sum_ideal[o];
        }
        r[k] = x;
    }
    saw_nan = __syncthreads_or(saw_nan);
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < P / 2; i += kMedianBlock) {
                const int lo = ((i / stride) * stride * 2) + (i % stride), hi = lo + stride;
                const bool up = ((lo & size) == 0);
                const double a = r[lo], b = r[hi];
                if ((a > b) == up) { r[lo] = b; r[hi] = a; }
            }
            __syncthreads();
        }
    // NCP: exact integer cents over the tree-summed ideal
    num = wave_sum_i64(num);
    for (int off = 32; off > 0; off >>= 1) den += __shfl_xor(den, off, 64);
    if ((tid & 63) == 0) { s_num[tid >> 6] = num; s_den[tid >> 6] = den; }
    __syncthreads();
    if (tid == 0) {
        long long n = 0;
        double d = 0.0;
        for (int i = 0; i < kMedianBlock / kWave; ++i) { n += s_num[i]; d += s_den[i]; }
        ncp[env] = ((double)n / 100.0) / (d <= 0.0 ? 1.0 : d);
        const double med = (K & 1) ? r[K / 2] : (r[K / 2 - 1] + r[K / 2]) * 0.5;
        akncp[env] = (days > 0.0 && !saw_nan) ? med : __builtin_nan("");
    }
}
