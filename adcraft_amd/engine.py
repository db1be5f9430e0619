"""StepEngine: thin object wrapper over the C ABI (include/adcraft_engine.h).

One engine = N environments x K keywords resident on one MI355X.  The per-step hot path of
the reference (adcraft/gymnasium_kw_env.py:160-269 -> adcraft/bidding_simulation.py:170-234)
is ONE call here for all environments.  numpy in / numpy out; device-resident variants for
consumers that keep actions and observations in HBM.
"""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import (MODEL_EXPLICIT, MODEL_IMPLICIT, P_A, P_B, P_BCTR, P_COUNT, P_REV_MEAN, P_REV_STD, P_SCTR,  # noqa: F401
                   P_VOL_MEAN, P_VOL_STD, check, ptr)

_OUT_SPEC = (("impressions", np.int32, True), ("buyside_clicks", np.int32, True),
             ("sellside_conversions", np.int32, True), ("cost", np.float32, True), ("revenue", np.float32, True),
             ("reward", np.float64, False), ("cumulative_profit", np.float64, False), ("days_passed", np.int32, False),
             ("terminated", np.uint8, False), ("truncated", np.uint8, False))


_COUNT_NAMES = ("impressions", "buyside_clicks", "sellside_conversions")


def _out_offsets(lib, handle):
    off, total = (C.c_size_t * 10)(), C.c_size_t()
    check(lib.adc_engine_out_offsets(handle, off, C.byref(total)))
    return list(off), total.value


def _views_at(block, offsets, N, K, names):
    """numpy views of a byte block at the engine's output offsets"""
    out = {}
    for (name, dt, per_kw), off in zip(_OUT_SPEC, offsets):
        if name in names:
            count = N * K if per_kw else N
            out[name] = block[off:off + count * np.dtype(dt).itemsize].view(dt).reshape((N, K) if per_kw else (N,))
    return out


def _alloc_outputs(alloc, N, K, compact, offsets, block_bytes):
    """the step outputs of one engine as views of ONE page-locked block laid out like the engine's device block, so that they
    come back in one transfer (adc_engine_out_offsets).  With compact counts the three count arrays are uint16 views [N, K] of
    a [N, 3, K] array the device packs (adc_step_out.counts_u16) and no int32 counts are transferred."""
    names = [n for n, _, _ in _OUT_SPEC if not (compact and n in _COUNT_NAMES)]
    out = _views_at(alloc((block_bytes,), np.uint8), offsets, N, K, names)
    if not compact:
        return out, None, None
    packed, overflow = alloc((N, 3, K), np.uint16), alloc((1,), np.int32)
    for i, name in enumerate(_COUNT_NAMES):
        out[name] = packed[:, i, :]
    return out, packed, overflow


def _out_struct(out, packed, overflow, b0, b1, small=None):
    """adc_step_out over rows b0:b1 of the output arrays (small: this part's own per-env arrays)"""
    src = lambda name, per_kw: (out[name][b0:b1] if per_kw or small is None else small[name]).ctypes.data   # noqa: E731
    if packed is None:
        return _ffi.StepOut(*(src(name, per_kw) for name, _, per_kw in _OUT_SPEC), None, None)
    ptrs = [None if name in _COUNT_NAMES else src(name, per_kw) for name, _, per_kw in _OUT_SPEC]
    return _ffi.StepOut(*ptrs, packed[b0:b1].ctypes.data, overflow[b0:b0 + 1].ctypes.data if overflow.size > 1 else overflow.ctypes.data)


def _is_buffer(a, buf):
    """a is the page-locked array buf itself (or a full view of it): nothing to stage"""
    return isinstance(a, np.ndarray) and a.dtype == buf.dtype and a.size == buf.size and a.flags.c_contiguous \
        and a.__array_interface__["data"][0] == buf.__array_interface__["data"][0]


def _check_overflow(overflow):
    if overflow is not None and overflow.any():
        overflow[...] = 0
        raise OverflowError("a keyword count exceeded 65535: construct the engine / env with compact_counts=False")


class StepEngine:
    def __init__(self, num_envs, num_keywords, model=MODEL_IMPLICIT, *, device_id=0, max_days=60,
                 loss_threshold=10000.0, drift=(0.03, 0.03, 0.03), drift_enabled=False, impression_thresh=0.05,
                 auto_reset=False, env_id_base=0, seed=0, compact_counts=False):
        self._h = None
        self._lib = _ffi.lib()
        self.num_envs, self.num_keywords, self.model = int(num_envs), int(num_keywords), int(model)
        self.max_days = int(max_days)
        cfg = _ffi.Config(C.sizeof(_ffi.Config), int(device_id), self.num_envs, self.num_keywords, self.model,
                          int(max_days), float(loss_threshold), float(drift[0]), float(drift[1]), float(drift[2]),
                          1 if drift_enabled else 0, float(impression_thresh), 1 if auto_reset else 0,
                          int(env_id_base), int(seed) & 0xFFFFFFFFFFFFFFFF)
        h = C.c_void_p()
        check(self._lib.adc_engine_create(C.byref(cfg), C.byref(h)))
        self._h = h
        N, K = self.num_envs, self.num_keywords
        # step I/O buffers live in page-locked host memory: observations DMA straight into these numpy arrays
        self._pinned = []
        self.compact_counts = bool(compact_counts)
        self.out, self._counts_u16, self._overflow = _alloc_outputs(self._pinned_array, N, K, self.compact_counts,
                                                                    *_out_offsets(self._lib, self._h))
        self._out = _out_struct(self.out, self._counts_u16, self._overflow, 0, N)
        self._flat_io = None
        self._bids_stage = self._pinned_array((N, K), np.float32)
        self._budget_stage = self._pinned_array((N,), np.float32)

    def _pinned_array(self, shape, dtype):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        check(self._lib.adc_host_alloc(max(nbytes, 1), C.byref(p)))
        self._pinned.append(p.value)
        buf = (C.c_char * max(nbytes, 1)).from_address(p.value)
        a = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        a[...] = 0
        return a

    # ---- lifecycle
    def close(self):
        if self._h is not None:
            self._lib.adc_engine_destroy(self._h)
            self._h = None
            self.out, self._bids_stage, self._budget_stage, self._flat_io = {}, None, None, None      # drop views before freeing
            self._counts_u16, self._overflow = None, None
            for p in self._pinned:
                self._lib.adc_host_free(p)
            self._pinned = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- keyword state
    def set_params(self, param_id, values):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(values, dtype=np.float32),
                                                 (self.num_envs, self.num_keywords)))
        check(self._lib.adc_engine_set_params(self._h, int(param_id), a.ctypes.data))

    def set_all_params(self, planes):
        """planes: float array [8][N][K] (or broadcastable to it)"""
        planes = np.asarray(planes, dtype=np.float32)
        for p in range(P_COUNT):
            self.set_params(p, planes[p])

    def set_env_params(self, env, planes_8k):
        a = np.ascontiguousarray(planes_8k, dtype=np.float32).reshape(P_COUNT, self.num_keywords)
        check(self._lib.adc_engine_set_env_params(self._h, int(env), a.ctypes.data))

    def get_params(self, param_id):
        a = np.zeros((self.num_envs, self.num_keywords), dtype=np.float32)
        check(self._lib.adc_engine_get_params(self._h, int(param_id), a.ctypes.data))
        return a

    def get_all_params(self):
        return np.stack([self.get_params(p) for p in range(P_COUNT)])

    def reset(self, env_mask=None, seeds=None):
        m = None if env_mask is None else np.ascontiguousarray(env_mask, dtype=np.uint8)
        s = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        if m is not None and m.shape != (self.num_envs,):
            raise ValueError("env_mask must have shape (num_envs,)")
        if s is not None and s.shape != (self.num_envs,):
            raise ValueError("seeds must have shape (num_envs,)")
        check(self._lib.adc_engine_reset(self._h, ptr(m), ptr(s)))

    QUANTITIES = ("vol", "ave_cpc", "std_cpc", "bctr", "sctr", "rpsc", "std_rpsc")

    def generate_keywords(self, table, no_vol_prob=0.0, env_mask=None, serial=0):
        """draw every (masked) env's keyword set on the device from a quantile table (dict of columns
        count_/min_/median_/max_<quantity>, as the reference's DataFrame); see adc_engine_generate_keywords"""
        q = _ffi.Quantiles()
        keep = []
        for i, name in enumerate(self.QUANTITIES):
            col = lambda c: np.asarray(table[f"{c}_{name}"].to_numpy() if hasattr(table[f"{c}_{name}"], "to_numpy")  # noqa: E731
                                       else table[f"{c}_{name}"], dtype=np.float64)
            sel = col("count") > 0 if f"count_{name}" in table and name != "vol" else np.ones(len(col("min")), bool)
            arrs = [np.ascontiguousarray(col(c)[sel], dtype=np.float32) for c in ("min", "median", "max")]
            keep.append(arrs)
            q.buckets[i] = arrs[0].size
            q.mins[i], q.medians[i], q.maxs[i] = (a.ctypes.data for a in arrs)
        m = None if env_mask is None else np.ascontiguousarray(env_mask, dtype=np.uint8)
        check(self._lib.adc_engine_generate_keywords(self._h, C.byref(q), float(no_vol_prob), int(serial), ptr(m)))

    def generate_explicit_keywords(self, env_mask=None, serial=0):
        """draw every (masked) env's EXPLICIT keyword set on the device: the law of sample_random_keywords
        (gymnasium_kw_utils.py:113-156), from each env's own Philox key; see adc_engine_generate_explicit_keywords"""
        m = None if env_mask is None else np.ascontiguousarray(env_mask, dtype=np.uint8)
        check(self._lib.adc_engine_generate_explicit_keywords(self._h, int(serial), ptr(m)))

    def set_limits(self, max_days, loss_threshold):
        check(self._lib.adc_engine_set_limits(self._h, int(max_days), float(loss_threshold)))
        self.max_days = int(max_days)

    def set_general_model(self, max_bidders=30, participation_rate=0.6, num_winners=1):
        """model=2 (the reference's default ImplicitKeyword): bidder pool and number of winning placements"""
        check(self._lib.adc_engine_set_general_model(self._h, int(max_bidders), float(participation_rate), int(num_winners)))

    def set_drift(self, enabled, drift=(0.03, 0.03, 0.03)):
        check(self._lib.adc_engine_set_drift(self._h, 1 if enabled else 0, float(drift[0]), float(drift[1]), float(drift[2])))

    def set_drift_mask(self, mask):
        """which keywords move at each update_keywords(): None (every keyword), bool [K] (the same for every env) or
        [N, K].  An explicit selection (the reference's prefix rule for a partial updater_mask is
        gymnasium_kw_utils.effective_updater_mask); the pending update moves under the selection it was scheduled with.
        Does not switch drift on: set_drift does."""
        if mask is None:
            check(self._lib.adc_engine_set_drift_mask(self._h, None))
            return
        m = np.asarray(mask)
        if m.shape not in ((self.num_keywords,), (self.num_envs, self.num_keywords)):
            raise ValueError(f"drift mask must have shape ({self.num_keywords},) or ({self.num_envs}, {self.num_keywords}), got {m.shape}")
        m = np.ascontiguousarray(np.broadcast_to(m.astype(bool), (self.num_envs, self.num_keywords)), dtype=np.uint8)
        check(self._lib.adc_engine_set_drift_mask(self._h, m.ctypes.data))

    def set_env_drift(self, rates):
        """per-env drift magnitudes (vol, ctr, cvr - updater_params' numbers): None (set_drift's scalars), [3] (every env)
        or [N, 3]; the pending update moves under the magnitudes it was scheduled with"""
        if rates is None:
            check(self._lib.adc_engine_set_env_drift(self._h, None))
            return
        r = np.asarray(rates, dtype=np.float32)
        if r.shape not in ((3,), (self.num_envs, 3)):
            raise ValueError(f"drift rates must have shape (3,) or ({self.num_envs}, 3), got {r.shape}")
        r = np.ascontiguousarray(np.broadcast_to(r, (self.num_envs, 3)))
        check(self._lib.adc_engine_set_env_drift(self._h, r.ctypes.data))

    def get_rng_state(self):
        k = np.zeros(self.num_envs, dtype=np.uint64)
        t = np.zeros(self.num_envs, dtype=np.uint32)
        check(self._lib.adc_engine_get_rng_state(self._h, k.ctypes.data, t.ctypes.data))
        return k, t

    def set_rng_state(self, keys=None, ticks=None):
        k = None if keys is None else np.ascontiguousarray(keys, dtype=np.uint64)
        t = None if ticks is None else np.ascontiguousarray(ticks, dtype=np.uint32)
        check(self._lib.adc_engine_set_rng_state(self._h, ptr(k), ptr(t)))

    def get_episode_state(self):
        d = np.zeros(self.num_envs, dtype=np.int32)
        c = np.zeros(self.num_envs, dtype=np.float64)
        check(self._lib.adc_engine_get_episode_state(self._h, d.ctypes.data, c.ctypes.data))
        return d, c

    def set_episode_state(self, day=None, cum_profit=None):
        d = None if day is None else np.ascontiguousarray(day, dtype=np.int32)
        c = None if cum_profit is None else np.ascontiguousarray(cum_profit, dtype=np.float64)
        check(self._lib.adc_engine_set_episode_state(self._h, ptr(d), ptr(c)))

    # ---- the hot path
    def _actions(self, bids, budget):
        if not _is_buffer(bids, self._bids_stage):
            self._bids_stage[...] = np.asarray(bids, dtype=np.float32).reshape(-1, self.num_keywords) if np.ndim(bids) else bids
        if not _is_buffer(budget, self._budget_stage):
            self._budget_stage[...] = budget
        return self._bids_stage, self._budget_stage

    def action_buffers(self):
        """(bids [N, K], budget [N]) page-locked arrays: fill them in place and pass them to step() to skip the staging copy"""
        return self._bids_stage, self._budget_stage

    def step(self, bids, budget, copy=True):
        """host in / host out, synchronous.  Returns dict of numpy arrays (views of reused buffers if copy=False)."""
        b, g = self._actions(bids, budget)
        check(self._lib.adc_engine_step(self._h, b.ctypes.data, g.ctypes.data, C.byref(self._out)))
        _check_overflow(self._overflow)
        return {k: v.copy() for k, v in self.out.items()} if copy else self.out

    def outcomes_replay(self, env, bids_k, budget, steps_back=1, tape=None):
        """the paid clicks of one step of env `env` (steps_back = 1: its last), one by one, in the reference's order
        (adc_engine_outcomes_replay): dict of keyword, timestep, cost (dollars), revenue (dollars, -1 = no conversion) and
        share_volume [K].  An earlier step can be replayed while drift is off and nothing has changed the parameters since.
        With a ReplayTape the step is the one the tape describes (adc_engine_outcomes_replay_tape: parity against the reference's
        recorded BiddingOutcomes); nothing of the engine's state is touched either way."""
        K = self.num_keywords
        bids = np.ascontiguousarray(bids_k, dtype=np.float32).reshape(K)
        share = np.zeros(K, np.int32)
        n = C.c_int64(0)
        cap = 4096
        while True:
            kw, ts = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
            cost, rev = np.zeros(cap, np.float64), np.zeros(cap, np.float64)
            if tape is None:
                check(self._lib.adc_engine_outcomes_replay(self._h, int(env), int(steps_back), bids.ctypes.data, float(budget), cap, kw.ctypes.data,
                                                           ts.ctypes.data, cost.ctypes.data, rev.ctypes.data, C.byref(n), share.ctypes.data))
            else:
                check(self._lib.adc_engine_outcomes_replay_tape(self._h, int(env), bids.ctypes.data, float(budget), C.byref(tape.struct), cap,
                                                                kw.ctypes.data, ts.ctypes.data, cost.ctypes.data, rev.ctypes.data, C.byref(n),
                                                                share.ctypes.data))
            if n.value <= cap:
                m = n.value
                return dict(keyword=kw[:m], timestep=ts[:m], cost=cost[:m], revenue=rev[:m], share_volume=share)
            cap = int(n.value)

    def step_flat(self, flat_actions):
        """FlatArrayWrapper-layout step: actions float32 [N, K+1] = [budget, bids...] -> (flat_obs [N, 5K+2], reward,
        terminated, truncated); the returned arrays are views of page-locked buffers, valid until the next step"""
        N, K = self.num_envs, self.num_keywords
        if self._flat_io is None:
            self._flat_io = (self._pinned_array((N, K + 1), np.float32), self._pinned_array((N, 5 * K + 2), np.float32))
        act, obs = self._flat_io
        act[...] = flat_actions
        check(self._lib.adc_engine_step_flat(self._h, act.ctypes.data, obs.ctypes.data, self.out["reward"].ctypes.data,
                                             self.out["terminated"].ctypes.data, self.out["truncated"].ctypes.data))
        return obs, self.out["reward"], self.out["terminated"], self.out["truncated"]

    def step_async(self, bids_ptr, budget_ptr, out_struct=None):
        """enqueue a host-in / host-out step and return (adc_engine_step_async); the buffers (page-locked) must stay
        untouched until wait()"""
        check(self._lib.adc_engine_step_async(self._h, bids_ptr, budget_ptr, C.byref(self._out if out_struct is None else out_struct)))

    def step_flat_async(self, act_ptr, obs_ptr, reward_ptr, term_ptr, trunc_ptr):
        check(self._lib.adc_engine_step_flat_async(self._h, act_ptr, obs_ptr, reward_ptr, term_ptr, trunc_ptr))

    def wait(self):
        check(self._lib.adc_engine_wait(self._h))

    def step_replay(self, bids, budget, tape, copy=True):
        b, g = self._actions(bids, budget)
        check(self._lib.adc_engine_step_replay(self._h, b.ctypes.data, g.ctypes.data, C.byref(tape.struct), C.byref(self._out)))
        _check_overflow(self._overflow)
        return {k: v.copy() for k, v in self.out.items()} if copy else self.out

    def step_device(self, d_bids=None, d_budget=None):
        """asynchronous; None = the engine's staging buffers (see sample_actions / device_buffer)."""
        check(self._lib.adc_engine_step_device(self._h, d_bids, d_budget))

    def fetch(self, copy=True):
        check(self._lib.adc_engine_fetch(self._h, C.byref(self._out)))
        _check_overflow(self._overflow)
        return {k: v.copy() for k, v in self.out.items()} if copy else self.out

    def synchronize(self):
        check(self._lib.adc_engine_synchronize(self._h))

    def update_keywords(self):
        check(self._lib.adc_engine_update_keywords(self._h))

    def sample_actions(self, bid_lo=0.30, bid_hi=1.00, budget=1.0e9):
        check(self._lib.adc_engine_sample_actions(self._h, bid_lo, bid_hi, budget))

    def flat_obs_enable(self, on=True):
        check(self._lib.adc_engine_flat_obs_enable(self._h, 1 if on else 0))

    def set_flat_actions_device(self, d_flat_ptr):
        """device pointer to float32 [N][K+1] = [budget, bids...] -> the engine's staging buffers (async)"""
        check(self._lib.adc_engine_set_flat_actions_device(self._h, d_flat_ptr))

    def device_buffer(self, buffer_id):
        p = C.c_void_p()
        n = C.c_size_t()
        check(self._lib.adc_engine_device_buffer(self._h, int(buffer_id), C.byref(p), C.byref(n)))
        return p.value, n.value

    def stream(self):
        p = C.c_void_p()
        check(self._lib.adc_engine_stream(self._h, C.byref(p)))
        return p.value

    # ---- measurement / metrics
    def profile_enable(self, on=True, every=1):
        """HIP events around the kernels of every `every`-th step (recording them costs ~16 us a step: sample when timing)"""
        check(self._lib.adc_engine_profile_sample_every(self._h, int(every)))
        check(self._lib.adc_engine_profile_enable(self._h, 1 if on else 0))

    def profile_read(self):
        """(ms_fast_pass, ms_exact_pass_and_tail, ms_metric_accumulate), measured steps - summed since the last read"""
        ms = (C.c_double * 3)()
        n = C.c_int64()
        check(self._lib.adc_engine_profile_read(self._h, ms, C.byref(n)))
        return tuple(ms), n.value

    def profile_records(self):
        """event records issued since the engine was created (four per bracketed step; none while profiling is off)"""
        n = C.c_int64()
        check(self._lib.adc_engine_profile_records(self._h, C.byref(n)))
        return n.value

    def walk_stats(self, reset=False):
        """k_step_click_walk's counters on this device: [walked, list overflowed, campaign stopped, other hand-overs] (adc_debug_walk_stats)"""
        out = np.zeros(4, dtype=np.int64)
        check(self._lib.adc_debug_walk_stats(self._h, out.ctypes.data, 1 if reset else 0))
        return out

    def direct_days(self, reset=False):
        """env-days handed to k_step_rest_of_day without the row kernel, on this device (adc_debug_direct_days)"""
        out = np.zeros(1, dtype=np.int64)
        check(self._lib.adc_debug_direct_days(self._h, out.ctypes.data, 1 if reset else 0))
        return int(out[0])

    def env_groups(self):
        """how many env groups (streams) the last IMPLICIT step ran as (adc_engine_env_groups); scheduling only"""
        n = C.c_int32(1)
        check(self._lib.adc_engine_env_groups(self._h, C.byref(n)))
        return n.value

    def set_env_groups(self, groups):
        """0: the engine chooses how many env groups a step runs as; 1..4: that many (adc_engine_set_env_groups)"""
        check(self._lib.adc_engine_set_env_groups(self._h, int(groups)))

    def step_kernel_name(self):
        """the first-pass kernel of the last step (the one profile_read()'s first duration times)"""
        return self._lib.adc_engine_step_kernel_name(self._h).decode()

    def metrics_enable(self, on=True):
        check(self._lib.adc_engine_metrics_enable(self._h, 1 if on else 0))

    def metrics_reset(self):
        check(self._lib.adc_engine_metrics_reset(self._h))

    def ideal_profit(self, n_samples=2048, bid_grid=None):
        """max expected profit per keyword from the current parameters (experiment_metrics.py:20-61), dollars [N, K];
        bid_grid defaults to the notebooks' np.arange(0.01, 3.00, 0.01).  IMPLICIT and EXPLICIT keywords (EXPLICIT: the
        curves of bid_curves_build, get_explicit_kw_bid_cpc_impressions' law; n_samples <= 2^20)"""
        grid = np.ascontiguousarray(np.arange(0.01, 3.00, 0.01) if bid_grid is None else bid_grid, dtype=np.float64)
        out = np.zeros((self.num_envs, self.num_keywords), dtype=np.float64)
        check(self._lib.adc_engine_ideal_profit(self._h, int(n_samples), grid.ctypes.data, grid.size, out.ctypes.data))
        return out

    def metrics_read(self):
        kp = np.zeros(self.num_keywords, dtype=np.int64)
        sc = np.zeros(8, dtype=np.int64)
        check(self._lib.adc_engine_metrics_read(self._h, kp.ctypes.data, sc.ctypes.data))
        return kp, sc


    # ---- device-resident callers of the step: per-step ideal profit and the baseline bidders --------------------
    def bid_curves_build(self, n_samples=2048, bid_grid=None):
        """cache the bid curves of every keyword on the device: get_implicit_kw_bid_cpc_impressions (experiment_metrics.py:20-37,
        8 bytes per grid point) or, for EXPLICIT keywords, get_explicit_kw_bid_cpc_impressions (:10-17: the two middle normals
        of the n_samples cost draws and the keyword's impression parameters, 16 bytes per keyword)"""
        grid = np.ascontiguousarray(np.arange(0.01, 3.00, 0.01) if bid_grid is None else bid_grid, dtype=np.float64)
        check(self._lib.adc_engine_bid_curves_build(self._h, int(n_samples), grid.ctypes.data, grid.size))
        self._bid_grid = grid

    def bid_curves_fetch(self):
        """the cached curves as host arrays (impression_rate, cpc), each [N, K, n_bids]: the doubles the ideal kernels evaluate"""
        nb = self._bid_grid.size
        ir = np.zeros((self.num_envs, self.num_keywords, nb), np.float64)
        cpc = np.zeros((self.num_envs, self.num_keywords, nb), np.float64)
        check(self._lib.adc_engine_bid_curves_fetch(self._h, ir.ctypes.data, cpc.ctypes.data))
        return ir, cpc

    def bid_curves_contenders(self):
        """(count [N, K] (65535 = the whole grid), grid indices [N, K, cap], margin intervals [N, K, cap, 2]) of the curve points
        the per-step ideal chooses from (IMPLICIT and EXPLICIT curves)"""
        cap = C.c_int32(0)
        check(self._lib.adc_engine_bid_curves_contenders(self._h, None, None, C.byref(cap)))
        n = np.zeros((self.num_envs, self.num_keywords), np.uint16)
        ent = np.zeros((self.num_envs, self.num_keywords, cap.value, 6), np.uint32)
        check(self._lib.adc_engine_bid_curves_contenders(self._h, n.ctypes.data, ent.ctypes.data, C.byref(cap)))
        return n, ent[..., 4].astype(np.int32), ent[..., 0:2].copy().view(np.float32)

    def ideal_step(self, fetch=True):
        """get_max_expected_bid_profits for the current parameters against the cached curves (IMPLICIT or EXPLICIT); with
        metrics enabled the ideal is also accumulated.  Returns (ideal [N, K] dollars, argmax index [N, K]) or None if not fetch."""
        if not fetch:
            check(self._lib.adc_engine_ideal_step(self._h, None, None))
            return None
        ideal = np.zeros((self.num_envs, self.num_keywords), dtype=np.float64)
        best = np.zeros((self.num_envs, self.num_keywords), dtype=np.int32)
        check(self._lib.adc_engine_ideal_step(self._h, ideal.ctypes.data, best.ctypes.data))
        return ideal, best

    def policy_oracle(self, budget=100000.0):
        """next action := the grid bid of maximum expected profit (after ideal_step)"""
        check(self._lib.adc_engine_policy_oracle(self._h, float(budget)))

    def agent_init(self, default_rpc=3.0, seeds=None):
        sd = None if seeds is None else np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (self.num_envs,)))
        check(self._lib.adc_engine_agent_init(self._h, float(default_rpc), None if sd is None else sd.ctypes.data))

    def agent_update(self, clicks=None, conversions=None, revenue=None):
        if clicks is None and conversions is None and revenue is None:
            check(self._lib.adc_engine_agent_update(self._h, None, None, None))
            return
        shape = (self.num_envs, self.num_keywords)
        c = np.ascontiguousarray(np.asarray(clicks).reshape(shape), dtype=np.int32)
        v = np.ascontiguousarray(np.asarray(conversions).reshape(shape), dtype=np.int32)
        r = np.ascontiguousarray(np.asarray(revenue).reshape(shape), dtype=np.float32)
        check(self._lib.adc_engine_agent_update(self._h, c.ctypes.data, v.ctypes.data, r.ctypes.data))

    def agent_act(self, budget_override=0.0, replay_uniforms=None):
        u = None
        if replay_uniforms is not None:
            u = np.ascontiguousarray(np.asarray(replay_uniforms, dtype=np.float64).reshape(self.num_envs, self.num_keywords))
        check(self._lib.adc_engine_agent_act(self._h, float(budget_override), None if u is None else u.ctypes.data))

    def agent_step(self, budget_override=0.0):
        check(self._lib.adc_engine_agent_step(self._h, float(budget_override)))

    def agent_state(self):
        shape = (self.num_envs, self.num_keywords)
        st = dict(ave_rpc=np.zeros(shape, np.float32), num_rpc_obs=np.zeros(shape, np.int32), ave_sctr=np.zeros(shape, np.float32),
                  num_sctr_obs=np.zeros(shape, np.int32), max_bids=np.zeros(shape, np.float64))
        check(self._lib.adc_engine_agent_state(self._h, *(st[k].ctypes.data for k in ("ave_rpc", "num_rpc_obs", "ave_sctr",
                                                                                      "num_sctr_obs", "max_bids"))))
        return st

    # ---- NaiveInterpolationStrategy, one agent per env (parts/kernel_interp_agent.inc) ----------------------------------
    def interp_init(self, threshold=-0.2, bid_step=0.03, allowed_bids=None, capacity=0, seeds=None):
        """empty caches, own last bid 0.01; capacity 0 = min(300, max_days + 1) interpolation points per keyword"""
        g = np.ascontiguousarray(np.linspace(0.01, 3.00, 300) if allowed_bids is None else allowed_bids, dtype=np.float64).reshape(-1)
        sd = None if seeds is None else np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (self.num_envs,)))
        check(self._lib.adc_engine_interp_init(self._h, float(threshold), float(bid_step), g.ctypes.data, int(g.size), int(capacity),
                                               None if sd is None else sd.ctypes.data))

    def interp_set_allowed_bids(self, allowed_bids):
        g = np.ascontiguousarray(allowed_bids, dtype=np.float64).reshape(-1)
        check(self._lib.adc_engine_interp_set_allowed_bids(self._h, g.ctypes.data, int(g.size)))

    def interp_update(self, prev_bids=None, clicks=None, cost=None, conversions=None, revenue=None):
        """host arrays [N, K] (all five), or none = the agent's own last bids and the engine's last observation"""
        if all(x is None for x in (prev_bids, clicks, cost, conversions, revenue)):
            check(self._lib.adc_engine_interp_update(self._h, None, None, None, None, None))
            return
        shape = (self.num_envs, self.num_keywords)
        b = np.ascontiguousarray(np.asarray(prev_bids, dtype=np.float64).reshape(shape))
        c = np.ascontiguousarray(np.asarray(clicks).reshape(shape), dtype=np.int32)
        x = np.ascontiguousarray(np.asarray(cost).reshape(shape), dtype=np.float32)
        v = np.ascontiguousarray(np.asarray(conversions).reshape(shape), dtype=np.int32)
        r = np.ascontiguousarray(np.asarray(revenue).reshape(shape), dtype=np.float32)
        check(self._lib.adc_engine_interp_update(self._h, b.ctypes.data, c.ctypes.data, x.ctypes.data, v.ctypes.data, r.ctypes.data))

    def interp_act(self, budget_override=0.0, replay_uniforms=None):
        u = None
        if replay_uniforms is not None:
            u = np.ascontiguousarray(np.asarray(replay_uniforms, dtype=np.float64).reshape(self.num_envs, self.num_keywords))
        check(self._lib.adc_engine_interp_act(self._h, float(budget_override), None if u is None else u.ctypes.data))

    def interp_step(self, budget_override=0.0):
        check(self._lib.adc_engine_interp_step(self._h, float(budget_override)))

    def interp_state(self):
        """rpc / sctr caches, max_observed and the last bid's grid index (-1: none) [N, K]; the last act's budget, profit_beliefs, cost_beliefs [N] (float64)"""
        shape, n = (self.num_envs, self.num_keywords), self.num_envs
        st = dict(ave_rpc=np.zeros(shape, np.float32), num_rpc_obs=np.zeros(shape, np.int32), ave_sctr=np.zeros(shape, np.float32),
                  num_sctr_obs=np.zeros(shape, np.int32), max_observed=np.zeros(shape, np.float64), bid_index=np.zeros(shape, np.int32),
                  budget=np.zeros(n, np.float64),
                  profit_beliefs=np.zeros(n, np.float64), cost_beliefs=np.zeros(n, np.float64))
        check(self._lib.adc_engine_interp_state(self._h, *(st[k].ctypes.data for k in (
            "ave_rpc", "num_rpc_obs", "ave_sctr", "num_sctr_obs", "max_observed", "bid_index", "budget", "profit_beliefs",
            "cost_beliefs"))))
        return st

    def interp_entries(self):
        """the interpolation points: dict of [N, K] list lengths and [N, K, capacity] slots (ascending cents in the first n)"""
        cap = C.c_int32(0)
        check(self._lib.adc_engine_interp_entries(self._h, C.byref(cap), *([None] * 8)))
        c, shape = cap.value, (self.num_envs, self.num_keywords)
        st = dict(n_clicks=np.zeros(shape, np.int32), clicks_cent=np.zeros((c,) + shape, np.uint16), ave_clicks=np.zeros((c,) + shape, np.float32),
                  clicks_count=np.zeros((c,) + shape, np.int32), n_cpc=np.zeros(shape, np.int32), cpc_cent=np.zeros((c,) + shape, np.uint16),
                  ave_cpc=np.zeros((c,) + shape, np.float64), cpc_count=np.zeros((c,) + shape, np.int32))
        check(self._lib.adc_engine_interp_entries(self._h, None, *(st[k].ctypes.data for k in (
            "n_clicks", "clicks_cent", "ave_clicks", "clicks_count", "n_cpc", "cpc_cent", "ave_cpc", "cpc_count"))))
        for k in ("clicks_cent", "ave_clicks", "clicks_count", "cpc_cent", "ave_cpc", "cpc_count"):
            st[k] = np.moveaxis(st[k], 0, -1)
        st["capacity"] = c
        return st

    def get_actions(self):
        bids = np.zeros((self.num_envs, self.num_keywords), np.float32)
        budget = np.zeros(self.num_envs, np.float32)
        check(self._lib.adc_engine_get_actions(self._h, bids.ctypes.data, budget.ctypes.data))
        return bids, budget

    # ---- the MLP policy, one agent per env (parts/kernel_mlp_policy.inc, parts/mlp_api.inc; baselines/mlp_policy.py builds `policy`) ----
    def mlp_init(self, policy, seeds=None, deterministic=None):
        """shapes and options of an MLPPolicy, then its weights; deterministic (if given) overrides the policy's own flag"""
        cfg = policy.config(self.num_keywords, deterministic)
        sd = None if seeds is None else np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (self.num_envs,)))
        frames = int(getattr(policy, "frames", 1))
        if getattr(policy, "gru", None) is not None:
            check(self._lib.adc_engine_mlp_init_recurrent(self._h, C.byref(cfg), None if sd is None else sd.ctypes.data, policy.gru_width))
        elif frames == 1:
            check(self._lib.adc_engine_mlp_init(self._h, C.byref(cfg), None if sd is None else sd.ctypes.data))
        else:
            check(self._lib.adc_engine_mlp_init_frames(self._h, C.byref(cfg), None if sd is None else sd.ctypes.data, frames))
        self._td3_norm = self._sac_norm = None                   # (the TD3 normalisers, if any, ended with their trainer)
        self._mlp = policy
        self._frames = frames
        self._members = 0                   # (a population does not survive a re-initialisation)
        self._learners = 0
        self.mlp_set_weights(policy)

    def _mlp_policy(self):
        """the policy given to mlp_init"""
        if getattr(self, "_mlp", None) is None:
            raise _ffi.EngineStateError("mlp_init has not been called")
        return self._mlp

    def _upload_layers(self, set_layer, networks):
        """every layer of `networks` - pairs of (the arguments that name a network, its layers) - through one set_*_layer function"""
        for where, layers in networks:
            for i, (w, b) in enumerate(layers):
                check(set_layer(self._h, *where, i, w.ctypes.data, b.ctypes.data))

    def mlp_set_weights(self, policy):
        """upload every layer, the normalisation vectors and log_std of `policy` (same shapes as at mlp_init): a trainer's
        update between days; nothing else of the agent changes"""
        if policy.shapes() != self._mlp_policy().shapes():
            raise ValueError(f"mlp_set_weights: the policy's shapes {policy.shapes()} are not those given to mlp_init "
                             f"{self._mlp.shapes()} (layers, value layers, free log_std, normalisation)")
        self._upload_layers(self._lib.adc_engine_mlp_set_layer, (((0,), policy.layers), ((1,), policy.value_layers)))
        if getattr(policy, "gru", None) is not None:
            check(self._lib.adc_engine_mlp_set_gru(self._h, *(a.ctypes.data for a in policy.gru)))
        if policy.shift is not None:
            check(self._lib.adc_engine_mlp_set_norm(self._h, policy.shift.ctypes.data, policy.scale.ctypes.data))
        if policy.log_std is not None:
            check(self._lib.adc_engine_mlp_set_log_std(self._h, policy.log_std.ctypes.data))

    def mlp_set_log_std(self, log_std):
        """the free log_std vector [K + 1] alone (the exploration noise of an off-policy trainer); nothing else changes"""
        ls = np.ascontiguousarray(log_std, dtype=np.float32)
        if ls.shape != (self.num_keywords + 1,):
            raise ValueError("mlp_set_log_std: K + 1 entries")
        check(self._lib.adc_engine_mlp_set_log_std(self._h, ls.ctypes.data))

    def mlp_set_deterministic(self, on=True):
        check(self._lib.adc_engine_mlp_set_deterministic(self._h, 1 if on else 0))

    def mlp_set_squash(self, lo=None, hi=None):
        """the squashed action: with lo / hi [K + 1] (flat action order: budget, bids) the env is given lo + 0.5 (hi - lo)
        (tanh(u) + 1) in place of the sampled action u; the record, mlp_last and the log-probability keep u.  Both None: off"""
        self._set_bounds(self._lib.adc_engine_mlp_set_squash, "mlp_set_squash", lo, hi)

    def mlp_learners_set_squash(self, lo=None, hi=None):
        """mlp_set_squash for learners (mlp_learners first): one pair of bounds lo / hi [K + 1] shared by all members.  Both
        None: off.  mlp_learners, mlp_population and mlp_init drop it."""
        self._set_bounds(self._lib.adc_engine_mlp_learners_set_squash, "mlp_learners_set_squash", lo, hi)

    EXPLORE_MODES = {"gaussian": 0, "random": 1}

    def _set_bounds(self, fn, name, lo, hi):
        """lo / hi [K + 1] (or scalars) through one of the squash or bounds setters; both None: off"""
        if lo is None and hi is None:
            check(fn(self._h, None, None))
            return
        if lo is None or hi is None:
            raise ValueError(name + ": lo and hi, or neither")
        a = self.num_keywords + 1
        lo, hi = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float32), (a,))) for v in (lo, hi))
        check(fn(self._h, lo.ctypes.data, hi.ctypes.data))

    def mlp_set_bounds(self, lo=None, hi=None):
        """the bounded act (csrc/adc_mlp.h "bounded"), TD3's: with lo / hi [K + 1] (or scalars; flat action order: budget, bids)
        the action is n = clamp(tanh(mean) + exp(log_std) z, -1, 1) in units of the box (tanh(mean) for a deterministic act), the
        env is given lo + 0.5 (hi - lo) (n + 1), and the record and mlp_last hold n; logp is +0.  Both None: off"""
        self._set_bounds(self._lib.adc_engine_mlp_set_bounds, "mlp_set_bounds", lo, hi)

    def mlp_learners_set_bounds(self, lo=None, hi=None):
        """mlp_set_bounds for learners (mlp_learners first): one pair of bounds shared by all members.  Both None: off.
        mlp_learners, mlp_population and mlp_init drop it."""
        self._set_bounds(self._lib.adc_engine_mlp_learners_set_bounds, "mlp_learners_set_bounds", lo, hi)

    def mlp_set_explore(self, mode="gaussian"):
        """the bounded act's exploration: "gaussian", or "random" - the warm-up: n uniform in (-1, 1) from the word the act's
        normal would have been made from (the ticks move as ever; a deterministic act stays tanh(mean))"""
        if mode not in self.EXPLORE_MODES:
            raise ValueError(f"unknown exploration mode {mode!r}: 'gaussian' or 'random'")
        check(self._lib.adc_engine_mlp_set_explore(self._h, self.EXPLORE_MODES[mode]))

    def mlp_bounds(self):
        """dict of bounded (bool), explore ("gaussian" / "random") and, while the bounds are on, lo and hi [K + 1]"""
        a = self.num_keywords + 1
        lo, hi, on, mode = np.zeros(a, np.float32), np.zeros(a, np.float32), C.c_int32(0), C.c_int32(0)
        check(self._lib.adc_engine_mlp_get_bounds(self._h, lo.ctypes.data, hi.ctypes.data, C.byref(on), C.byref(mode)))
        out = dict(bounded=bool(on.value), explore="random" if mode.value == 1 else "gaussian")
        if on.value:
            out.update(lo=lo, hi=hi)
        return out

    def mlp_act(self, budget_override=0.0, replay_normals=None):
        z = None
        if replay_normals is not None:
            z = np.ascontiguousarray(np.asarray(replay_normals, dtype=np.float32).reshape(self.num_envs, self.num_keywords + 1))
        check(self._lib.adc_engine_mlp_act(self._h, float(budget_override), None if z is None else z.ctypes.data))

    def mlp_step(self, budget_override=0.0):
        """act + the env's step on the device (recorded when rollout_enable is on)"""
        check(self._lib.adc_engine_mlp_step(self._h, float(budget_override)))

    def mlp_last(self):
        """the last act: mean, log_std, action [N, K+1] (flat action order: budget, bids), logp, value [N]"""
        n, a = self.num_envs, self.num_keywords + 1
        st = dict(mean=np.zeros((n, a), np.float32), log_std=np.zeros((n, a), np.float32), action=np.zeros((n, a), np.float32),
                  logp=np.zeros(n, np.float32), value=np.zeros(n, np.float32))
        check(self._lib.adc_engine_mlp_last(self._h, *(st[k].ctypes.data for k in ("mean", "log_std", "action", "logp", "value"))))
        return st

    def mlp_set_norm(self, shift, scale):
        """the policy's normalisation vectors [D] (every member's under per-member normalisers; running moments are left alone)"""
        D = self.mlp_input_size()
        sh, sc = (np.ascontiguousarray(a, dtype=np.float32) for a in (shift, scale))
        if sh.shape != (D,) or sc.shape != (D,):
            raise ValueError(f"mlp_set_norm: shift and scale have {D} entries")
        check(self._lib.adc_engine_mlp_set_norm(self._h, sh.ctypes.data, sc.ctypes.data))

    def mlp_frames(self):
        """the frames of the policy's input row (MLPPolicy(frames=H); 1 without an observation history)"""
        f = C.c_int32(0)
        check(self._lib.adc_engine_mlp_frames(self._h, C.byref(f)))
        return f.value

    def mlp_input_size(self):
        """D = frames * (5K + 2): the width of the network input, a record's obs row and the normalisation vectors"""
        return int(getattr(self, "_frames", 1)) * (5 * self.num_keywords + 2)

    def mlp_history_state(self):
        """the observation history: dict(hist float32 [N, H, 5K+2] raw frames, last, from int32 [N]); None without one (frames = 1)"""
        h = self.mlp_frames()
        if h == 1:
            return None
        n, d0 = self.num_envs, 5 * self.num_keywords + 2
        st = {"hist": np.zeros((n, h, d0), np.float32), "last": np.zeros(n, np.int32), "from": np.zeros(n, np.int32)}
        check(self._lib.adc_engine_mlp_history_get(self._h, st["hist"].ctypes.data, st["last"].ctypes.data, st["from"].ctypes.data))
        return st

    def mlp_set_history_state(self, state):
        """restore what mlp_history_state returned (None: nothing to restore); a resumed run continues bit for bit"""
        h = self.mlp_frames()
        if state is None:
            if h != 1:
                raise ValueError("mlp_set_history_state: the policy has an observation history and the state has none")
            return
        n, d0 = self.num_envs, 5 * self.num_keywords + 2
        hist = np.ascontiguousarray(state["hist"], dtype=np.float32)
        last, frm = (np.ascontiguousarray(state[k], dtype=np.int32) for k in ("last", "from"))
        if h == 1 or hist.shape != (n, h, d0) or last.shape != (n,) or frm.shape != (n,):
            raise ValueError(f"mlp_set_history_state: hist [N, {h}, 5K+2], last and from [N] of a policy with frames = {h}")
        check(self._lib.adc_engine_mlp_history_set(self._h, hist.ctypes.data, last.ctypes.data, frm.ctypes.data))

    # ---- the recurrent policy's state (parts/gru_api.inc; csrc/adc_gru.h) ----
    def mlp_gru_width(self):
        """the width G of the policy's GRU cell (MLPPolicy(gru=...)); 0: the policy is feed-forward"""
        g = C.c_int32(0)
        check(self._lib.adc_engine_mlp_gru_width(self._h, C.byref(g)))
        return g.value

    def mlp_hidden_state(self):
        """the cell's state: dict(h float32 [N, 2, G] (slot = episode day & 1), last, from int32 [N]); None for a feed-forward policy"""
        g = self.mlp_gru_width()
        if g == 0:
            return None
        n = self.num_envs
        st = {"h": np.zeros((n, 2, g), np.float32), "last": np.zeros(n, np.int32), "from": np.zeros(n, np.int32)}
        check(self._lib.adc_engine_mlp_hidden_get(self._h, st["h"].ctypes.data, st["last"].ctypes.data, st["from"].ctypes.data))
        return st

    def mlp_set_hidden_state(self, state):
        """restore what mlp_hidden_state returned (None: nothing to restore); a resumed run continues bit for bit"""
        g = self.mlp_gru_width()
        if state is None:
            if g != 0:
                raise ValueError("mlp_set_hidden_state: the policy is recurrent and the state holds no hidden state")
            return
        n = self.num_envs
        h = np.ascontiguousarray(state["h"], dtype=np.float32)
        last, frm = (np.ascontiguousarray(state[k], dtype=np.int32) for k in ("last", "from"))
        if g == 0 or h.shape != (n, 2, g) or last.shape != (n,) or frm.shape != (n,):
            raise ValueError(f"mlp_set_hidden_state: h [N, 2, {g}], last and from [N] of a policy with a cell of width {g}")
        check(self._lib.adc_engine_mlp_hidden_set(self._h, h.ctypes.data, last.ctypes.data, frm.ctypes.data))

    def mlp_hidden_forget(self):
        """every env's next act starts from a zero state (es_perturb does this too)"""
        check(self._lib.adc_engine_mlp_hidden_forget(self._h))

    def mlp_agent_state(self):
        """(keys uint64 [N], ticks uint32 [N]) of the agents' own streams; every act moves a tick on by one"""
        k, t = np.zeros(self.num_envs, np.uint64), np.zeros(self.num_envs, np.uint32)
        check(self._lib.adc_engine_mlp_agent_state(self._h, k.ctypes.data, t.ctypes.data))
        return k, t

    def mlp_bootstrap_value(self):
        v = np.zeros(self.num_envs, np.float32)
        check(self._lib.adc_engine_mlp_bootstrap_value(self._h, v.ctypes.data))
        return v

    # ---- policy populations and the evolution strategy over them (parts/kernel_es.inc, parts/mlp_api.inc, parts/es_api.inc; baselines/es_trainer.py) ----
    def mlp_population(self, members, member_of_env=None):
        """`members` copies of the policy network's layers, each starting as the centre policy; member_of_env [N] (default
        env // (N // members)) says whose weights an env runs.  0 turns the population off.  The value network, log_std and
        the normalisation stay shared."""
        m = None if member_of_env is None else np.ascontiguousarray(member_of_env, dtype=np.int32)
        if m is not None and m.shape != (self.num_envs,):
            raise ValueError("member_of_env: one member per env")
        check(self._lib.adc_engine_mlp_population(self._h, int(members), None if m is None else m.ctypes.data))
        self._members = int(members)
        if int(members) > 0:
            self._learners = 0              # (a population drops learners)

    def mlp_set_member(self, member, policy):
        """the policy layers of `policy` (same shapes as at mlp_init) into one member"""
        if [w.shape for w, _ in policy.layers] != [w.shape for w, _ in self._mlp_policy().layers]:
            raise ValueError("mlp_set_member: the policy's layer shapes are not those given to mlp_init")
        if [a.shape for a in (getattr(policy, "gru", None) or ())] != [a.shape for a in (getattr(self._mlp, "gru", None) or ())]:
            raise ValueError("mlp_set_member: the policy's cell is not the shape of the one given to mlp_init")
        self._upload_layers(self._lib.adc_engine_mlp_set_member_layer, (((int(member),), policy.layers),))
        if getattr(policy, "gru", None) is not None:
            check(self._lib.adc_engine_mlp_set_member_gru(self._h, int(member), *(a.ctypes.data for a in policy.gru)))

    def mlp_param_count(self):
        n = C.c_int64(0)
        check(self._lib.adc_engine_mlp_param_count(self._h, C.byref(n)))
        return n.value

    def mlp_params(self):
        """the centre policy's parameters in the flat order (layers in order, W input-major then b; a recurrent policy's cell -
        Wi, bi, Wh, bh - stands in front of its output layer)"""
        flat = np.zeros(self.mlp_param_count(), np.float32)
        check(self._lib.adc_engine_mlp_get_params(self._h, flat.ctypes.data))
        return flat

    def mlp_member_params(self, member):
        flat = np.zeros(self.mlp_param_count(), np.float32)
        check(self._lib.adc_engine_mlp_get_member_params(self._h, int(member), flat.ctypes.data))
        return flat

    # ---- learners: per-member policy layers, value layers and log_std (parts/mlp_api.inc; the members pg_pop_* trains) ----------
    def mlp_learners(self, members):
        """`members` learners, each with its own policy layers, value layers and log_std, each starting as the centre policy;
        member m owns the envs [m N / M, (m + 1) N / M).  0 turns the mode off.  Excludes mlp_population."""
        check(self._lib.adc_engine_mlp_learners(self._h, int(members)))
        self._learners = int(members)
        if int(members) > 0:
            self._members = 0

    def mlp_set_learner(self, member, policy):
        """every layer of both networks and log_std of `policy` (same shapes as at mlp_init) into one learner"""
        if policy.shapes() != self._mlp_policy().shapes():
            raise ValueError(f"mlp_set_learner: the policy's shapes {policy.shapes()} are not those given to mlp_init {self._mlp.shapes()}")
        m = int(member)
        self._upload_layers(self._lib.adc_engine_mlp_set_learner_layer, (((m, 0), policy.layers), ((m, 1), policy.value_layers)))
        if policy.log_std is not None:
            check(self._lib.adc_engine_mlp_set_learner_log_std(self._h, int(member), policy.log_std.ctypes.data))

    def mlp_set_learner_log_std(self, member, log_std):
        """one learner's free log_std vector [K + 1] alone (its exploration noise under td3_pop_*); the next act reads it"""
        ls = np.ascontiguousarray(log_std, dtype=np.float32)
        if ls.shape != (self.num_keywords + 1,):
            raise ValueError("mlp_set_learner_log_std: K + 1 entries")
        check(self._lib.adc_engine_mlp_set_learner_log_std(self._h, int(member), ls.ctypes.data))

    def mlp_learner_params(self, member):
        """one learner's parameters in the trainer's flat order theta[Q]: policy layers, value layers, log_std"""
        theta = np.zeros(self.mlp_learner_param_count(), np.float32)
        check(self._lib.adc_engine_mlp_get_learner_params(self._h, int(member), theta.ctypes.data))
        return theta

    def mlp_learner_param_count(self):
        """Q: the parameters of both networks and log_std of the policy given to mlp_init"""
        q = C.c_int64(0)
        cfg = self._mlp_policy().config(self.num_keywords)
        if self._lib.adc_pg_param_count_host(C.byref(cfg), self.num_keywords, C.byref(q)) != _ffi.ADC_OK:
            raise ValueError("bad policy configuration")
        # (the host twin counts one frame's inputs: an observation history widens both first layers)
        firsts = [net[0][0].shape[1] for net in (self._mlp.layers, self._mlp.value_layers) if net]
        return q.value + (self.mlp_input_size() - (5 * self.num_keywords + 2)) * sum(firsts)

    ES_SHAPINGS = {"centered_rank": _ffi.ES_CENTERED_RANK, "raw": _ffi.ES_RAW}
    ES_OPTIMISERS = {"adam": _ffi.ES_ADAM, "sgd": _ffi.ES_SGD}

    @classmethod
    def es_config(cls, sigma=0.02, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, l2=0.0, shaping="centered_rank", optimiser="adam", seed=0):
        c = _ffi.ESConfig()
        c.struct_size = C.sizeof(_ffi.ESConfig)
        c.sigma, c.lr, c.beta1, c.beta2, c.eps, c.l2 = sigma, lr, beta1, beta2, eps, l2
        c.shaping, c.optimiser, c.seed = cls.ES_SHAPINGS[shaping], cls.ES_OPTIMISERS[optimiser], int(seed)
        msg = C.c_char_p()
        if _ffi.lib().adc_es_config_check(C.byref(c), C.byref(msg)) != _ffi.ADC_OK:
            raise ValueError((msg.value or b"bad ES configuration").decode())
        return c

    def es_init(self, **options):
        """an evolution strategy over the population (csrc/adc_es.h); options as es_config's.  theta starts as the centre."""
        cfg = self.es_config(**options)
        check(self._lib.adc_engine_es_init(self._h, C.byref(cfg)))

    def es_perturb(self):
        """members = theta +- sigma * noise of the current generation; returns zeroed; accumulation on"""
        check(self._lib.adc_engine_es_perturb(self._h))

    def es_fitness(self):
        """[members] float64: the mean over a member's envs of the reward summed over the days since es_perturb"""
        f = np.zeros(getattr(self, "_members", 0), np.float64)
        check(self._lib.adc_engine_es_fitness(self._h, f.ctypes.data))
        return f

    def es_update(self, fitness=None):
        """one generation's step from the device's fitness (or `fitness` [members]); dict of generation, fitness_mean / max /
        min, grad_norm, theta_norm"""
        f = None if fitness is None else np.ascontiguousarray(fitness, dtype=np.float64)
        members = getattr(self, "_members", 0)
        if f is not None and members and f.shape != (members,):
            raise ValueError("fitness: one value per member")
        st = _ffi.ESStats()
        check(self._lib.adc_engine_es_update(self._h, None if f is None else f.ctypes.data, C.byref(st)))
        return {k: getattr(st, k) for k, _ in _ffi.ESStats._fields_}

    def es_state(self, state=None):
        """get (no argument): dict of theta, m, v [P] float32 and generation; set: such a dict - the run continues bit for bit"""
        if state is None:
            P = self.mlp_param_count()
            st = dict(theta=np.zeros(P, np.float32), m=np.zeros(P, np.float32), v=np.zeros(P, np.float32))
            g = C.c_int64(0)
            check(self._lib.adc_engine_es_state_get(self._h, st["theta"].ctypes.data, st["m"].ctypes.data, st["v"].ctypes.data, C.byref(g)))
            st["generation"] = g.value
            return st
        P = self.mlp_param_count()
        arr = [np.ascontiguousarray(state[k], dtype=np.float32) for k in ("theta", "m", "v")]
        if any(a.shape != (P,) for a in arr):
            raise ValueError(f"es_state: theta, m and v have {P} entries")
        check(self._lib.adc_engine_es_state_set(self._h, arr[0].ctypes.data, arr[1].ctypes.data, arr[2].ctypes.data, int(state["generation"])))

    # ---- policy-gradient training over the rollout record (parts/kernel_pg.inc; baselines/pg_trainer.py drives it) ----------
    PG_OPTIMISERS = {"adam": _ffi.PG_ADAM, "sgd": _ffi.PG_SGD}

    @classmethod
    def pg_config(cls, gamma=0.99, lam=0.95, eps_clip=0.2, vf_coef=0.5, ent_coef=0.0, reward_scale=1.0, normalize_advantages=True,
                  max_grad_norm=0.5, optimiser="adam", lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, minibatch_envs=0):
        """an adc_pg_config (csrc/adc_pg.h); eps_clip <= 0: no clip; max_grad_norm 0: off; minibatch_envs 0: all envs"""
        c = _ffi.PGConfig()
        c.struct_size = C.sizeof(_ffi.PGConfig)
        c.gamma, c.lambda_, c.eps_clip, c.vf_coef, c.ent_coef, c.reward_scale = gamma, lam, eps_clip, vf_coef, ent_coef, reward_scale
        c.normalize_advantages, c.max_grad_norm = 1 if normalize_advantages else 0, max_grad_norm
        if optimiser not in cls.PG_OPTIMISERS:
            raise ValueError(f"unknown optimiser {optimiser!r}: 'adam' or 'sgd'")
        c.optimiser, c.lr, c.beta1, c.beta2, c.eps, c.minibatch_envs = cls.PG_OPTIMISERS[optimiser], lr, beta1, beta2, eps, int(minibatch_envs)
        msg = C.c_char_p()
        if _ffi.lib().adc_pg_config_check(C.byref(c), C.byref(msg)) != _ffi.ADC_OK:
            raise ValueError((msg.value or b"bad policy-gradient configuration").decode())
        return c

    def pg_init(self, **options):
        """policy-gradient training of the policy given to mlp_init over the rollout record (rollout_enable(T, obs=True) first);
        options as pg_config's.  theta starts as the device's weights."""
        cfg = self.pg_config(**options)
        check(self._lib.adc_engine_pg_init(self._h, C.byref(cfg)))

    def pg_param_count(self):
        n = C.c_int64(0)
        check(self._lib.adc_engine_pg_param_count(self._h, C.byref(n)))
        return n.value

    # (`prefix`: pg or pg_pop - the family of the entry points and the public method's name in a message; `member`: a
    #  population's member, None for the single learner.  The host side is shared in the same way: parts/pg_core.inc)
    def _pg(self, prefix, name):
        return getattr(self._lib, f"adc_engine_{prefix}_{name}")

    def _learner_count(self):
        return max(getattr(self, "_learners", 0), 1)

    @staticmethod
    def _pg_stats(st):
        return {k: getattr(st, k) for k, _ in _ffi.PGStats._fields_}

    def _pg_advantages(self, prefix, fetch):
        check(self._pg(prefix, "advantages")(self._h))
        if not fetch:
            return None
        t = C.c_int32(0)
        check(self._lib.adc_engine_rollout_fetch(self._h, C.byref(t), *([None] * 7)))
        adv, ret = np.zeros((t.value, self.num_envs), np.float32), np.zeros((t.value, self.num_envs), np.float32)
        check(self._pg(prefix, "advantages_fetch")(self._h, adv.ctypes.data, ret.ctypes.data))
        return adv, ret

    def _pg_update(self, prefix, st, epochs, queued):
        check(self._pg(prefix, "update_queued" if queued else "update")(self._h, int(epochs), st))

    def _pg_state(self, prefix, member, state):
        who = () if member is None else (int(member),)
        Q = self.pg_param_count() if member is None else self.mlp_learner_param_count()
        if state is None:
            st = dict(theta=np.zeros(Q, np.float32), m=np.zeros(Q, np.float32), v=np.zeros(Q, np.float32))
            n = C.c_int64(0)
            check(self._pg(prefix, "state_get")(self._h, *who, st["theta"].ctypes.data, st["m"].ctypes.data, st["v"].ctypes.data, C.byref(n)))
            st["steps"] = n.value
            return st
        arr = [np.ascontiguousarray(state[k], dtype=np.float32) for k in ("theta", "m", "v")]
        if any(a.shape != (Q,) for a in arr):
            raise ValueError(f"{prefix}_state: theta, m and v have {Q} entries")
        check(self._pg(prefix, "state_set")(self._h, *who, arr[0].ctypes.data, arr[1].ctypes.data, arr[2].ctypes.data, int(state["steps"])))

    def pg_advantages(self, fetch=False):
        """GAE over the recorded days; fetch=True returns (adv, ret) [T, N] float32"""
        return self._pg_advantages("pg", fetch)

    def pg_minibatch(self, env_begin, env_count):
        """one gradient and one optimiser step over every recorded day of the envs [env_begin, env_begin + env_count)"""
        st = _ffi.PGStats()
        check(self._lib.adc_engine_pg_minibatch(self._h, int(env_begin), int(env_count), C.byref(st)))
        return self._pg_stats(st)

    def pg_update(self, epochs=1, queued=False):
        """advantages, then `epochs` x the minibatches in ascending env order; the last epoch's statistics.  queued=True: the
        whole update enqueued as one chain with one host wait (adc_engine_pg_update_queued) - the same bits"""
        st = _ffi.PGStats()
        self._pg_update("pg", C.byref(st), epochs, queued)
        return self._pg_stats(st)

    def pg_state(self, state=None):
        """get (no argument): dict of theta, m, v [Q] float32 and steps; set: such a dict - the run continues bit for bit"""
        return self._pg_state("pg", None, state)

    # ---- learner populations: M PPO / A2C learners in lock-step (parts/pg_api.inc; baselines/pg_trainer.py PGPopulationTrainer) ----
    @classmethod
    def pg_pop_configs(cls, configs, num_envs, members):
        """(ctypes array, count) from one dict of pg_config's options or `members` of them, checked by adc_pg_pop_config_check"""
        if isinstance(configs, dict):
            configs = [configs]
        built = [cls.pg_config(**c) for c in configs]
        arr = (_ffi.PGConfig * len(built))(*built)
        msg = C.c_char_p()
        if _ffi.lib().adc_pg_pop_config_check(arr, len(built), int(num_envs), int(members), C.byref(msg)) != _ffi.ADC_OK:
            raise ValueError((msg.value or b"bad population configuration").decode())
        return arr, len(built)

    def pg_pop_init(self, configs):
        """population training of the learners (mlp_learners, rollout_enable(T, obs=True) first); configs: one dict of
        pg_config's options shared by all members, or one per member.  Every member's theta starts as its device weights."""
        arr, count = self.pg_pop_configs(configs, self.num_envs, self._learner_count())
        check(self._lib.adc_engine_pg_pop_init(self._h, arr, count))

    def pg_pop_advantages(self, fetch=False):
        """GAE per env under its member's configuration; fetch=True returns (adv, ret) [T, N] float32"""
        return self._pg_advantages("pg_pop", fetch)

    def pg_pop_minibatch(self, index):
        """minibatch `index` of every member in the same launches; a list of M statistics dicts"""
        st = (_ffi.PGStats * self._learner_count())()
        check(self._lib.adc_engine_pg_pop_minibatch(self._h, int(index), st))
        return [self._pg_stats(x) for x in st]

    def pg_pop_update(self, epochs=1, queued=False):
        """advantages, then `epochs` x the minibatches ascending, all members at once; a list of M statistics dicts.
        queued=True: one chain, one host wait (adc_engine_pg_pop_update_queued) - the same bits"""
        st = (_ffi.PGStats * self._learner_count())()
        self._pg_update("pg_pop", st, epochs, queued)
        return [self._pg_stats(x) for x in st]

    def pg_pop_state(self, member, state=None):
        """one member's state.  get (no state): dict of theta, m, v [Q] float32 and steps; set: such a dict"""
        return self._pg_state("pg_pop", member, state)

    def pg_pop_set_config(self, member, **options):
        """a member's hyperparameters from the next call on (options as pg_config's; minibatch_envs may not change)"""
        cfg = self.pg_config(**options)
        check(self._lib.adc_engine_pg_pop_set_config(self._h, int(member), C.byref(cfg)))

    def pg_pop_copy(self, src, dst):
        """weights, optimiser moments and step count of member src into member dst, on the device"""
        check(self._lib.adc_engine_pg_pop_copy(self._h, int(src), int(dst)))

    # ---- PPO's adaptive KL penalty and value-loss clip (parts/kernel_pg_kl.inc; the law is csrc/adc_pg_kl.h) ----------------------
    @classmethod
    def pg_kl_config(cls, kl_coef=0.2, kl_target=0.01, adaptive=True, vf_clip=0.0, factor_up=0.0, factor_down=0.0):
        """an adc_pg_kl_config: kl_coef the starting coefficient of the analytic KL(pi_old || pi_new) in the loss; adaptive: after
        every update it is multiplied by factor_up (0: 1.5) when the last epoch's mean KL exceeds 2 kl_target, by factor_down
        (0: 0.5) when it is below 0.5 kl_target; vf_clip > 0 caps a sample's squared value error (0: off).  The defaults are
        RLlib's PPO's (kl_coeff 0.2, kl_target 0.01), configuration, not measurements."""
        c = _ffi.PGKLConfig()
        c.struct_size = C.sizeof(_ffi.PGKLConfig)
        c.kl_coef, c.kl_target, c.adaptive = float(kl_coef), float(kl_target), 1 if adaptive else 0
        c.factor_up, c.factor_down, c.vf_clip = float(factor_up), float(factor_down), float(vf_clip)
        msg = C.c_char_p()
        if _ffi.lib().adc_pg_kl_config_check(C.byref(c), C.byref(msg)) != _ffi.ADC_OK:
            raise ValueError((msg.value or b"bad KL penalty configuration").decode())
        return c

    def pg_kl_init(self, per_member=None, **options):
        """the KL penalty and the value-loss clip on the live PPO / A2C trainer (pg_init or pg_pop_init first); options as
        pg_kl_config's, shared by all learners - or per_member: a list of such dicts, one per learner of a population"""
        if per_member is not None and options:
            raise ValueError("pg_kl_init: options shared by all members, or per_member, not both")
        built = [self.pg_kl_config(**o) for o in per_member] if per_member is not None else [self.pg_kl_config(**options)]
        arr = (_ffi.PGKLConfig * len(built))(*built)
        check(self._lib.adc_engine_pg_kl_init(self._h, arr, len(built)))
        self._pg_kl_members = self._learner_count()

    def pg_kl_stats(self):
        """of the last minibatch or update: dict of kl, vf_clip_fraction, kl_coef (used), kl_coef_next - a list of them, one
        per learner, under a population"""
        st = (_ffi.PGKLStats * getattr(self, "_pg_kl_members", 1))()
        check(self._lib.adc_engine_pg_kl_stats(self._h, st))
        out = [{k: getattr(x, k) for k, _ in _ffi.PGKLStats._fields_} for x in st]
        return out if getattr(self, "_learners", 0) else out[0]

    def pg_kl_coef(self, member=0, value=None):
        """a learner's KL coefficient (float32), the add-on's whole state.  get (no value) or set"""
        if value is None:
            c = C.c_float(0.0)
            check(self._lib.adc_engine_pg_kl_coef_get(self._h, int(member), C.byref(c)))
            return np.float32(c.value)
        check(self._lib.adc_engine_pg_kl_coef_set(self._h, int(member), float(np.float32(value))))

    def pg_kl_old_dist(self):
        """the snapshot the last advantages call took: (mean_old [T, N, A], ls_old [T, N, A] with two heads, else [members, A])"""
        self.pg_kl_coef(0)                      # (refused here, by the add-on's own message, when it does not live)
        t = C.c_int32(0)
        check(self._lib.adc_engine_rollout_fetch(self._h, C.byref(t), *([None] * 7)))
        A = self.num_keywords + 1
        mean = np.zeros((t.value, self.num_envs, A), np.float32)
        two = self._mlp.log_std is None
        ls = np.zeros((t.value, self.num_envs, A) if two else (getattr(self, "_pg_kl_members", 1), A), np.float32)
        check(self._lib.adc_engine_pg_kl_old_dist_fetch(self._h, mean.ctypes.data, ls.ctypes.data))
        return mean, ls

    # ---- PPO's shuffled sample-level minibatches and target-KL early stop (parts/kernel_pg_shuffle.inc; csrc/adc_pg_shuffle.h) ----
    @classmethod
    def pg_shuffle_config(cls, minibatch_samples=64, seed=0, target_kl=0.0):
        """an adc_pg_shuffle_config: minibatch_samples recorded samples per minibatch, drawn from a new permutation of a learner's
        samples every epoch (RLlib's sgd_minibatch_size, Stable-Baselines3's batch_size); seed 0: the engine's; target_kl > 0 ends
        an update before the step of the first minibatch whose approx_kl exceeds 1.5 target_kl (0: never)"""
        c = _ffi.PGShuffleConfig()
        c.struct_size = C.sizeof(_ffi.PGShuffleConfig)
        c.minibatch_samples, c.seed, c.target_kl = int(minibatch_samples), int(seed), float(target_kl)
        msg = C.c_char_p()
        if _ffi.lib().adc_pg_shuffle_config_check(C.byref(c), C.byref(msg)) != _ffi.ADC_OK:
            raise ValueError((msg.value or b"bad shuffled-minibatch configuration").decode())
        return c

    def pg_shuffle_init(self, per_member=None, **options):
        """shuffled sample-level minibatches on the live PPO / A2C trainer (pg_init or pg_pop_init first); options as
        pg_shuffle_config's, shared by all learners - or per_member: a list of such dicts, one per learner of a population
        (minibatch_samples equal in all).  pg_update / pg_pop_update then run over them and honour target_kl."""
        if per_member is not None and options:
            raise ValueError("pg_shuffle_init: options shared by all members, or per_member, not both")
        built = [self.pg_shuffle_config(**o) for o in per_member] if per_member is not None else [self.pg_shuffle_config(**options)]
        arr = (_ffi.PGShuffleConfig * len(built))(*built)
        check(self._lib.adc_engine_pg_shuffle_init(self._h, arr, len(built)))
        self._pg_shuffle_members = self._learner_count()

    def pg_shuffle_epoch(self):
        """draw the order of a new epoch for every learner (after pg_advantages / pg_pop_advantages)"""
        check(self._lib.adc_engine_pg_shuffle_epoch(self._h))

    def pg_shuffle_minibatch(self, index):
        """minibatch `index` of the epoch's order: one gradient and - unless target_kl stops the learner - one step; the
        statistics dict, a list of them under a population"""
        st = (_ffi.PGStats * getattr(self, "_pg_shuffle_members", 1))()
        check(self._lib.adc_engine_pg_shuffle_minibatch(self._h, int(index), st))
        out = [self._pg_stats(x) for x in st]
        return out if getattr(self, "_learners", 0) else out[0]

    def pg_shuffle_order(self):
        """the order last drawn: (order, rows), uint32 [members, n_s] each - position i holds sample order[m, i] of learner m,
        which is row rows[m, i] of the record flattened to [T * N].  Refused once the advantages are stale (a day recorded,
        rollout_reset, a changed configuration): the order belongs to the days recorded when it was drawn"""
        self.pg_shuffle_stats()                 # (refused here, by the add-on's own message, when it does not live)
        t = C.c_int32(0)
        check(self._lib.adc_engine_rollout_fetch(self._h, C.byref(t), *([None] * 7)))
        M = getattr(self, "_pg_shuffle_members", 1)
        n_s = t.value * (self.num_envs // M)
        order, rows = np.zeros((M, n_s), np.uint32), np.zeros((M, n_s), np.uint32)
        check(self._lib.adc_engine_pg_shuffle_order_fetch(self._h, order.ctypes.data, rows.ctypes.data))
        return order, rows

    def pg_shuffle_stats(self):
        """of the last update (or the one in progress): dict of epochs_begun, minibatches_evaluated, steps_taken, stopped - a list
        of them, one per learner, under a population"""
        st = (_ffi.PGShuffleStats * getattr(self, "_pg_shuffle_members", 1))()
        check(self._lib.adc_engine_pg_shuffle_stats(self._h, st))
        out = [{k: getattr(x, k) for k, _ in _ffi.PGShuffleStats._fields_} for x in st]
        return out if getattr(self, "_learners", 0) else out[0]

    # ---- what the four off-policy front ends share (parts/offpolicy_core.inc).  `prefix`: td3, sac, td3_pop or sac_pop - the family of
    # the entry points and the public method's name in a message; `member`: a population's member, None for the solo trainers ----------
    def _off(self, prefix, name):
        return getattr(self._lib, f"adc_engine_{prefix}_{name}")

    def _off_set_critics(self, prefix, member, critics, action_norm, sync_targets):
        if len(critics) != 2:
            raise ValueError(f"{prefix}_set_critics: two critics")
        m = () if member is None else (int(member),)
        for i, layers in enumerate(critics):
            for l, (w, b) in enumerate(layers):
                w, b = np.ascontiguousarray(w, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
                check(self._off(prefix, "set_critic_layer")(self._h, *m, i, l, w.ctypes.data, b.ctypes.data))
        if action_norm is not None:
            sh, sc = (np.ascontiguousarray(a, dtype=np.float32) for a in action_norm)
            if sh.shape != (self.num_keywords + 1,) or sc.shape != sh.shape:
                raise ValueError("action_norm: shift and scale of K + 1 entries")
            check(self._off(prefix, "set_action_norm")(self._h, sh.ctypes.data, sc.ctypes.data))
        if sync_targets:
            check(self._off(prefix, "sync_targets")(self._h, *m))

    def _off_store(self, prefix):
        n = C.c_int64(0)
        check(self._off(prefix, "store")(self._h, C.byref(n)))
        return n.value

    def _off_buffer(self, prefix, member, fetch):
        pop = prefix.endswith("_pop")          # (the populations' buffer_info has the batch size; they fetch a member's ring alone)
        sz, wr, cap, b = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
        check(self._off(prefix, "buffer_info")(self._h, C.byref(sz), C.byref(wr), C.byref(cap), *((C.byref(b),) if pop else ())))
        st = dict(size=sz.value, written=wr.value, capacity=cap.value, **(dict(batch_size=b.value) if pop else {}))
        if fetch and (member is not None or not pop):
            n, D, A = sz.value, self.mlp_input_size(), self.num_keywords + 1
            st.update(x=np.zeros((n, D), np.float32), a=np.zeros((n, A), np.float32), r=np.zeros(n, np.float32), done=np.zeros(n, np.uint8),
                      x2=np.zeros((n, D), np.float32))
            if n:
                m = (int(member),) if pop else ()
                check(self._off(prefix, "buffer_fetch")(self._h, *m, 0, n, *(st[k].ctypes.data for k in ("x", "a", "r", "done", "x2"))))
            st["done"] = st["done"].astype(bool)
        return st

    def _off_buffer_load(self, prefix, member, buf, slot, written):
        D, A = self.mlp_input_size(), self.num_keywords + 1
        x, a, r, x2 = (np.ascontiguousarray(buf[k], dtype=np.float32) for k in ("x", "a", "r", "x2"))
        done = np.ascontiguousarray(buf["done"], dtype=np.uint8)
        n = r.shape[0]
        if x.shape != (n, D) or x2.shape != (n, D) or a.shape != (n, A) or done.shape != (n,):
            raise ValueError(f"{prefix}_buffer_load: x, x2 [n, D], a [n, K+1], r, done [n]")
        if written is None:
            written = buf.get("written", slot + n)
        m = () if member is None else (int(member),)
        check(self._off(prefix, "buffer_load")(self._h, *m, int(slot), n, x.ctypes.data, a.ctypes.data, r.ctypes.data, done.ctypes.data, x2.ctypes.data,
                                               int(written)))

    def _off_batch_indices(self, prefix, member, update):
        if member is None:
            b = C.c_int32(0)
            check(self._off(prefix, "batch_size")(self._h, C.byref(b)))       # (the engine says how many slots it will write)
            size, m = b.value, ()
        else:
            size, m = self._off_buffer(prefix, None, False)["batch_size"], (int(member),)
        idx = np.zeros(size, np.int32)
        check(self._off(prefix, "batch_indices")(self._h, *m, int(update), idx.ctypes.data))
        return idx

    def _off_update(self, prefix, stats_type, updates, members=None):
        """members None: one learner, its statistics dict; 0: a population, nothing fetched; M: a list of M dicts"""
        if members == 0:
            check(self._off(prefix, "update")(self._h, int(updates), None))
            return None
        st = stats_type() if members is None else (stats_type * members)()
        check(self._off(prefix, "update")(self._h, int(updates), C.byref(st) if members is None else st))
        out = [{k: getattr(x, k) for k, _ in stats_type._fields_} for x in ([st] if members is None else st)]
        return out[0] if members is None else out

    def _off_param_counts(self, prefix):
        p, q = C.c_int64(0), C.c_int64(0)
        check(self._off(prefix, "param_counts")(self._h, C.byref(p), C.byref(q)))
        return p.value, q.value

    def _off_state(self, prefix, names, member, state, counters):
        """names: the state's vectors in the entry points' order (TD3_STATE, SAC_STATE); counters: the integers after them"""
        P, Q = self._off_param_counts(prefix)
        size = lambda k: 3 if k == "log_alpha" else Q if "psi" in k else P
        m = () if member is None else (int(member),)
        if state is None:
            st = {k: np.zeros(size(k), np.float32) for k in names}
            got = [C.c_int64(0) for _ in counters]
            check(self._off(prefix, "state_get")(self._h, *m, *(st[k].ctypes.data for k in names), *(C.byref(c) for c in got)))
            st.update((k, c.value) for k, c in zip(counters, got))
            return st
        arr = [np.ascontiguousarray(state[k], dtype=np.float32) for k in names]
        if any(a.shape != (size(k),) for k, a in zip(names, arr)):
            raise ValueError(f"{prefix}_state: the actor's vectors have {P} entries, the critics' {Q}" + (", log_alpha 3" if "log_alpha" in names else ""))
        check(self._off(prefix, "state_set")(self._h, *m, *(a.ctypes.data for a in arr), *(int(state[k]) for k in counters)))

    # ---- off-policy (TD3) training over a replay ring filled from the record (parts/kernel_td3.inc, parts/td3_api.inc;
    # baselines/td3_trainer.py): the configuration and the init are TD3's, the rest wrappers of the _off_* helpers ----
    TD3_OPTIMISERS = {"adam": _ffi.TD3_ADAM, "sgd": _ffi.TD3_SGD}

    @classmethod
    def td3_config(cls, gamma=0.99, tau=0.005, policy_delay=2, target_noise=0.2, target_noise_clip=0.5, action_lo=0.0, action_hi=0.0,
                   reward_scale=1.0, batch_size=256, capacity=100000, critic_widths=(256, 256, 1), actor_lr=1e-3, critic_lr=1e-3,
                   beta1=0.9, beta2=0.999, eps=1e-8, optimiser="adam", max_grad_norm=0.0, seed=0):
        """an adc_td3_config (csrc/adc_td3.h) with Fujimoto et al.'s defaults; critic_widths: the outputs of every critic layer,
        the last 1; action_hi <= action_lo: the target action is not clamped; max_grad_norm 0: off; seed 0: the engine's"""
        c = _ffi.TD3Config()
        c.struct_size = C.sizeof(_ffi.TD3Config)
        c.gamma, c.tau, c.policy_delay, c.target_noise, c.target_noise_clip = gamma, tau, int(policy_delay), target_noise, target_noise_clip
        c.action_lo, c.action_hi, c.reward_scale, c.batch_size, c.capacity = action_lo, action_hi, reward_scale, int(batch_size), int(capacity)
        widths = [int(w) for w in critic_widths]
        if not 1 <= len(widths) <= 4:
            raise ValueError("critic_widths: 1 to 4 layers")
        c.n_critic_layers = len(widths)
        for i, w in enumerate(widths):
            c.critic_widths[i] = w
        if optimiser not in cls.TD3_OPTIMISERS:
            raise ValueError(f"unknown optimiser {optimiser!r}: 'adam' or 'sgd'")
        c.actor_lr, c.critic_lr, c.beta1, c.beta2, c.eps = actor_lr, critic_lr, beta1, beta2, eps
        c.optimiser, c.max_grad_norm, c.seed = cls.TD3_OPTIMISERS[optimiser], max_grad_norm, int(seed)
        msg = C.c_char_p()
        if _ffi.lib().adc_td3_config_check(C.byref(c), C.byref(msg)) != _ffi.ADC_OK:
            raise ValueError((msg.value or b"bad TD3 configuration").decode())
        return c

    def td3_init(self, **options):
        """TD3 on the policy given to mlp_init (free log_std head) over the rollout record (rollout_enable(T, obs=True) first);
        options as td3_config's.  theta starts as the device's policy; the critics are uploaded with td3_set_critics."""
        cfg = self.td3_config(**options)
        check(self._lib.adc_engine_td3_init(self._h, C.byref(cfg)))
        self._td3_norm = self._sac_norm = None                   # (the TD3 normalisers, if any, ended with their trainer)

    def td3_set_critics(self, critics, action_norm=None, sync_targets=True):
        """critics: two lists of (W [n_in, n_out], b [n_out]) float32 layers on the D + A inputs; action_norm: (shift, scale) [A]
        for the critics' action inputs; sync_targets: the targets become copies of the actor and the critics"""
        self._off_set_critics("td3", None, critics, action_norm, sync_targets)

    def td3_set_bounded(self, on=True):
        """bounded TD3 (csrc/adc_td3.h "bounded"; mlp_set_bounds first, no action_norm, no action_lo / action_hi, an empty
        ring): the critics read the act's n in [-1, 1], the target action is clamp(tanh(mu') + noise, -1, 1), the actor's
        gradient goes through tanh(mu)"""
        check(self._lib.adc_engine_td3_set_bounded(self._h, 1 if on else 0))

    def td3_pop_set_bounded(self, on=True):
        """td3_set_bounded for a population (mlp_learners_set_bounds first): all members at once"""
        check(self._lib.adc_engine_td3_pop_set_bounded(self._h, 1 if on else 0))

    def td3_bounded(self):
        """whether the TD3 learner (or population) on this engine is bounded"""
        on = C.c_int32(0)
        check(self._lib.adc_engine_td3_get_bounded(self._h, C.byref(on)))
        return bool(on.value)

    def td3_sync_targets(self):
        check(self._lib.adc_engine_td3_sync_targets(self._h))

    def td3_store(self):
        """the record's days not yet stored, into the ring; returns the transitions appended"""
        return self._off_store("td3")

    def td3_buffer(self, fetch=True):
        """dict of size, written, capacity and (fetch=True) the ring's slots [0, size): x [size, D], a [size, A], r [size],
        done [size] (bool), x2 [size, D]"""
        return self._off_buffer("td3", None, fetch)

    def td3_buffer_load(self, buf, slot=0, written=None):
        """the arrays of a td3_buffer() dict (or one of its kind) into the slots from `slot` on; written (default: the dict's, or
        slot + the count) becomes the ring's count of transitions stored so far"""
        self._off_buffer_load("td3", None, buf, slot, written)

    def td3_batch_indices(self, update):
        """the ring slots update number `update` reads at the ring's current size: [batch_size] int32"""
        return self._off_batch_indices("td3", None, update)

    def td3_update(self, updates=1):
        """`updates` critic updates and the delayed actor / target steps among them; the statistics of the last"""
        return self._off_update("td3", _ffi.TD3Stats, updates)

    def td3_param_counts(self):
        return self._off_param_counts("td3")

    TD3_STATE = ("theta", "psi", "theta_target", "psi_target", "m_theta", "v_theta", "m_psi", "v_psi")

    def td3_state(self, state=None):
        """get (no argument): dict of theta, theta_target, m_theta, v_theta [P], psi, psi_target, m_psi, v_psi [2 Qc] float32,
        updates and actor_steps; set: such a dict - with the ring (td3_buffer / td3_buffer_load) the run continues bit for bit"""
        return self._off_state("td3", self.TD3_STATE, None, state, ("updates", "actor_steps"))

    # ---- soft actor-critic over the same replay ring (parts/kernel_sac.inc, parts/sac_api.inc; baselines/sac_trainer.py): as TD3's,
    # wrappers of the _off_* helpers around SAC's own configuration and init ----------
    @classmethod
    def sac_config(cls, gamma=0.99, tau=0.005, target_update_interval=1, init_alpha=1.0, target_entropy=None, alpha_lr=3e-4, eps_sq=1e-6,
                   reward_scale=1.0, batch_size=256, capacity=100000, critic_widths=(256, 256, 1), actor_lr=3e-4, critic_lr=3e-4,
                   beta1=0.9, beta2=0.999, eps=1e-8, optimiser="adam", max_grad_norm=0.0, seed=0, num_keywords=None):
        """an adc_sac_config (csrc/adc_sac.h) with RLlib's SAC defaults; target_entropy None: -(num_keywords + 1); alpha_lr 0: alpha
        stays init_alpha; critic_widths: the outputs of every critic layer, the last 1; seed 0: the engine's"""
        c = _ffi.SACConfig()
        c.struct_size = C.sizeof(_ffi.SACConfig)
        if target_entropy is None:
            if num_keywords is None:
                raise ValueError("sac_config: target_entropy, or num_keywords for the default -(K + 1)")
            target_entropy = -float(num_keywords + 1)
        c.gamma, c.tau, c.target_update_interval, c.init_alpha, c.target_entropy = gamma, tau, int(target_update_interval), init_alpha, target_entropy
        c.alpha_lr, c.eps_sq, c.reward_scale, c.batch_size, c.capacity = alpha_lr, eps_sq, reward_scale, int(batch_size), int(capacity)
        widths = [int(w) for w in critic_widths]
        if not 1 <= len(widths) <= 4:
            raise ValueError("critic_widths: 1 to 4 layers")
        c.n_critic_layers = len(widths)
        for i, w in enumerate(widths):
            c.critic_widths[i] = w
        if optimiser not in cls.TD3_OPTIMISERS:
            raise ValueError(f"unknown optimiser {optimiser!r}: 'adam' or 'sgd'")
        c.actor_lr, c.critic_lr, c.beta1, c.beta2, c.eps = actor_lr, critic_lr, beta1, beta2, eps
        c.optimiser, c.max_grad_norm, c.seed = cls.TD3_OPTIMISERS[optimiser], max_grad_norm, int(seed)
        msg = C.c_char_p()
        if _ffi.lib().adc_sac_config_check(C.byref(c), C.byref(msg)) != _ffi.ADC_OK:
            raise ValueError((msg.value or b"bad SAC configuration").decode())
        return c

    def sac_init(self, **options):
        """SAC on the policy given to mlp_init (two heads, log-std clamp) with mlp_set_squash on, over the rollout record
        (rollout_enable(T, obs=True) first); options as sac_config's.  theta starts as the device's policy; the critics are
        uploaded with sac_set_critics."""
        options.setdefault("num_keywords", self.num_keywords)
        cfg = self.sac_config(**options)
        check(self._lib.adc_engine_sac_init(self._h, C.byref(cfg)))
        self._td3_norm = self._sac_norm = None

    def sac_set_critics(self, critics, sync_targets=True):
        """critics: two lists of (W [n_in, n_out], b [n_out]) float32 layers on the D + A inputs [x | tanh(u)]; sync_targets: the
        target critics become copies of the critics"""
        self._off_set_critics("sac", None, critics, None, sync_targets)

    def sac_sync_targets(self):
        check(self._lib.adc_engine_sac_sync_targets(self._h))

    def sac_store(self):
        """the record's days not yet stored, into the ring; returns the transitions appended"""
        return self._off_store("sac")

    def sac_buffer(self, fetch=True):
        """as td3_buffer: a holds the unsquashed actions u"""
        return self._off_buffer("sac", None, fetch)

    def sac_buffer_load(self, buf, slot=0, written=None):
        """as td3_buffer_load"""
        self._off_buffer_load("sac", None, buf, slot, written)

    def sac_batch_indices(self, update):
        """the ring slots update number `update` reads at the ring's current size: [batch_size] int32"""
        return self._off_batch_indices("sac", None, update)

    def sac_update(self, updates=1):
        """`updates` updates (critics, actor, temperature, targets); the statistics of the last"""
        return self._off_update("sac", _ffi.SACStats, updates)

    def sac_param_counts(self):
        return self._off_param_counts("sac")

    SAC_STATE = ("theta", "psi", "psi_target", "m_theta", "v_theta", "m_psi", "v_psi", "log_alpha")

    def sac_state(self, state=None):
        """get (no argument): dict of theta, m_theta, v_theta [P], psi, psi_target, m_psi, v_psi [2 Qc], log_alpha [3] (log_alpha and
        its two moments) float32, and updates; set: such a dict - with the ring (sac_buffer / sac_buffer_load) the run continues bit
        for bit"""
        return self._off_state("sac", self.SAC_STATE, None, state, ("updates",))

    # ---- TD3 learner populations: M off-policy learners in lock-step (parts/td3_pop_api.inc; baselines/td3_trainer.py
    # TD3PopulationTrainer): the _off_* helpers with a member; set_config and copy are the populations' own ----
    @classmethod
    def td3_pop_configs(cls, configs, num_envs, members):
        """(ctypes array, count) from one dict of td3_config's options or `members` of them, checked by adc_td3_pop_config_check"""
        if isinstance(configs, dict):
            configs = [configs]
        built = [cls.td3_config(**c) for c in configs]
        arr = (_ffi.TD3Config * len(built))(*built)
        msg = C.c_char_p()
        if _ffi.lib().adc_td3_pop_config_check(arr, len(built), int(num_envs), int(members), C.byref(msg)) != _ffi.ADC_OK:
            raise ValueError((msg.value or b"bad population configuration").decode())
        return arr, len(built)

    def _td3_pop_members(self):
        return max(getattr(self, "_learners", 0), 1)

    def td3_pop_init(self, configs):
        """population TD3 of the learners (mlp_learners, rollout_enable(T, obs=True) first); configs: one dict of td3_config's
        options shared by all members, or one per member (batch_size, capacity, critic_widths and policy_delay equal in all).
        Every member's theta starts as its device policy; the critics are uploaded with td3_pop_set_critics."""
        arr, count = self.td3_pop_configs(configs, self.num_envs, self._td3_pop_members())
        check(self._lib.adc_engine_td3_pop_init(self._h, arr, count))
        self._td3_norm = self._sac_norm = None                   # (the TD3 normalisers, if any, ended with their trainer)

    def td3_pop_set_critics(self, member, critics, action_norm=None, sync_targets=True):
        """one member's two critics (lists of (W [n_in, n_out], b [n_out]) on the D + A inputs); action_norm: (shift, scale) [A],
        shared by all members; sync_targets: the member's targets become copies of its actor and critics"""
        self._off_set_critics("td3_pop", member, critics, action_norm, sync_targets)

    def td3_pop_sync_targets(self, member=None):
        """member None: every member's targets"""
        check(self._lib.adc_engine_td3_pop_sync_targets(self._h, -1 if member is None else int(member)))

    def td3_pop_store(self):
        """the record's days not yet stored, into every member's ring; returns the transitions each member appended"""
        return self._off_store("td3_pop")

    def td3_pop_buffer(self, member=None, fetch=True):
        """dict of size, written, capacity, batch_size (the members' rings move together) and - for a member, fetch=True - its
        ring's slots [0, size) as td3_buffer's"""
        return self._off_buffer("td3_pop", member, fetch)

    def td3_pop_buffer_load(self, member, buf, slot=0, written=None):
        """the arrays of a td3_pop_buffer(member) dict (or one of its kind) into the member's slots from `slot` on; written
        becomes the count of transitions stored so far of every member's ring"""
        self._off_buffer_load("td3_pop", member, buf, slot, written)

    def td3_pop_batch_indices(self, member, update):
        """the slots of the member's ring its update number `update` reads at the ring's current size: [batch_size] int32"""
        return self._off_batch_indices("td3_pop", member, update)

    def td3_pop_update(self, updates=1, stats=True):
        """`updates` critic updates of every member and the delayed actor / target steps among them, all members in the same
        launches; a list of M statistics dicts (stats=False: None, and the call fetches nothing)"""
        return self._off_update("td3_pop", _ffi.TD3Stats, updates, self._td3_pop_members() if stats else 0)

    def td3_pop_param_counts(self):
        """(P, 2 Qc): the entries of a member's actor vectors and of its critics' vectors"""
        return self._off_param_counts("td3_pop")

    def td3_pop_state(self, member, state=None):
        """one member's state as td3_state's (the counters are the population's).  get (no state): the dict; set: such a dict"""
        return self._off_state("td3_pop", self.TD3_STATE, member, state, ("updates", "actor_steps"))

    def td3_pop_set_config(self, member, **options):
        """a member's hyperparameters from the next update on (options as td3_config's; the shared fields may not change)"""
        cfg = self.td3_config(**options)
        check(self._lib.adc_engine_td3_pop_set_config(self._h, int(member), C.byref(cfg)))

    def td3_pop_copy(self, src, dst, with_ring=False):
        """actor, critics, targets and optimiser moments of member src into member dst on the device (with_ring: its ring too);
        dst keeps its configuration, envs and exploration"""
        check(self._lib.adc_engine_td3_pop_copy(self._h, int(src), int(dst), 1 if with_ring else 0))

    # ---- SAC learner populations: M soft actor-critic learners in lock-step (parts/sac_pop_api.inc; baselines/sac_trainer.py
    # SACPopulationTrainer): the _off_* helpers with a member; set_config and copy are the populations' own ----
    @classmethod
    def sac_pop_configs(cls, configs, num_envs, members, num_keywords=None):
        """(ctypes array, count) from one dict of sac_config's options or `members` of them, checked by adc_sac_pop_config_check"""
        if isinstance(configs, dict):
            configs = [configs]
        built = [cls.sac_config(**dict(dict(num_keywords=num_keywords), **c)) for c in configs]
        arr = (_ffi.SACConfig * len(built))(*built)
        msg = C.c_char_p()
        if _ffi.lib().adc_sac_pop_config_check(arr, len(built), int(num_envs), int(members), C.byref(msg)) != _ffi.ADC_OK:
            raise ValueError((msg.value or b"bad population configuration").decode())
        return arr, len(built)

    def sac_pop_init(self, configs):
        """population SAC of the learners (mlp_learners, mlp_learners_set_squash and rollout_enable(T, obs=True) first; the
        two-headed policy with the log-std clamp); configs: one dict of sac_config's options shared by all members, or one per
        member (batch_size, capacity, critic_widths and target_update_interval equal in all).  Every member's theta starts as its
        device policy; the critics are uploaded with sac_pop_set_critics."""
        arr, count = self.sac_pop_configs(configs, self.num_envs, self._td3_pop_members(), self.num_keywords)
        check(self._lib.adc_engine_sac_pop_init(self._h, arr, count))
        self._td3_norm = self._sac_norm = None

    def sac_pop_set_critics(self, member, critics, sync_targets=True):
        """one member's two critics (lists of (W [n_in, n_out], b [n_out]) on the D + A inputs [x | tanh(u)]); sync_targets: the
        member's target critics become copies of its critics"""
        self._off_set_critics("sac_pop", member, critics, None, sync_targets)

    def sac_pop_sync_targets(self, member=None):
        """member None: every member's target critics"""
        check(self._lib.adc_engine_sac_pop_sync_targets(self._h, -1 if member is None else int(member)))

    def sac_pop_store(self):
        """the record's days not yet stored, into every member's ring; returns the transitions each member appended"""
        return self._off_store("sac_pop")

    def sac_pop_buffer(self, member=None, fetch=True):
        """dict of size, written, capacity, batch_size (the members' rings move together) and - for a member, fetch=True - its
        ring's slots [0, size) as sac_buffer's (a holds the unsquashed actions u)"""
        return self._off_buffer("sac_pop", member, fetch)

    def sac_pop_buffer_load(self, member, buf, slot=0, written=None):
        """the arrays of a sac_pop_buffer(member) dict (or one of its kind) into the member's slots from `slot` on; written
        becomes the count of transitions stored so far of every member's ring"""
        self._off_buffer_load("sac_pop", member, buf, slot, written)

    def sac_pop_batch_indices(self, member, update):
        """the slots of the member's ring its update number `update` reads at the ring's current size: [batch_size] int32"""
        return self._off_batch_indices("sac_pop", member, update)

    def sac_pop_update(self, updates=1, stats=True):
        """`updates` updates (critics, actor, temperature, targets) of every member, all members in the same launches; a list of
        M statistics dicts of the last (stats=False: None, and the call fetches nothing)"""
        return self._off_update("sac_pop", _ffi.SACStats, updates, self._td3_pop_members() if stats else 0)

    def sac_pop_param_counts(self):
        """(P, 2 Qc): the entries of a member's actor vectors and of its critics' vectors"""
        return self._off_param_counts("sac_pop")

    def sac_pop_state(self, member, state=None):
        """one member's state as sac_state's, log_alpha [3] its temperature cell's (the counter is the population's).  get (no
        state): the dict; set: such a dict"""
        return self._off_state("sac_pop", self.SAC_STATE, member, state, ("updates",))

    def sac_pop_set_config(self, member, **options):
        """a member's hyperparameters from the next update on (options as sac_config's; the shared fields may not change, and
        init_alpha is not read again: the temperature is state)"""
        options.setdefault("num_keywords", self.num_keywords)
        cfg = self.sac_config(**options)
        check(self._lib.adc_engine_sac_pop_set_config(self._h, int(member), C.byref(cfg)))

    def sac_pop_copy(self, src, dst, with_ring=False):
        """actor, critics, target critics, optimiser moments and the temperature cell of member src into member dst on the device
        (with_ring: its ring too); dst keeps its configuration, envs and seed"""
        check(self._lib.adc_engine_sac_pop_copy(self._h, int(src), int(dst), 1 if with_ring else 0))

    # ---- population-based training over the live pg_pop / td3_pop / sac_pop trainer (parts/pbt_api.inc; baselines/pbt.py PBTScheduler) ----
    PBT_IDS = {"pg": ("lr", "ent_coef", "eps_clip", "vf_coef"), "td3": ("actor_lr", "critic_lr", "target_noise", "tau", "sigma"),
               "sac": ("actor_lr", "critic_lr", "alpha_lr", "tau", "alpha", "target_entropy")}
    PBT_KINDS = {"pg": _ffi.PBT_PG, "td3": _ffi.PBT_TD3, "sac": _ffi.PBT_SAC}

    @classmethod
    def pbt_config(cls, kind, members, replace_count, tuned=(), bounds=None, factors=(0.8, 1.25), fitness_ema=0.0, with_ring=False, seed=0,
                   check=True):
        """an adc_pbt_config (csrc/adc_pbt.h) for a "pg", "td3" or "sac" population of `members`; tuned: names from PBT_IDS[kind];
        bounds: {name: (lo, hi)} for every tuned name ("sigma" and "alpha": in their own units, both positive, stored as float32
        logarithms - they live on the device and move in the log domain); factors: the
        two perturbation factors; seed 0: the engine's; check: run adc_pbt_config_check here (pbt_init leaves it to the engine,
        which knows the population)"""
        if kind not in cls.PBT_IDS:
            raise ValueError(f"unknown population kind {kind!r}: 'pg', 'td3' or 'sac'")
        ids, bounds = cls.PBT_IDS[kind], dict(bounds or {})
        c = _ffi.PBTConfig()
        c.struct_size = C.sizeof(_ffi.PBTConfig)
        c.replace_count, c.fitness_ema, c.with_ring, c.seed = int(replace_count), fitness_ema, 1 if with_ring else 0, int(seed)
        lo_f, hi_f = (float(x) for x in factors)
        if not (lo_f > 0 and hi_f > 0):
            raise ValueError("factors: two positive numbers")
        c.factor_lo, c.factor_hi = lo_f, hi_f
        c.log_factor_lo, c.log_factor_hi = np.float32(np.log(lo_f)), np.float32(np.log(hi_f))
        for name in tuned:
            if name not in ids:
                raise ValueError(f"{name!r} is not a tunable hyperparameter of a {kind} population: {ids}")
            if name not in bounds:
                raise ValueError(f"bounds: (lo, hi) for {name!r}")
            h, (lo, hi) = ids.index(name), bounds[name]
            c.tuned_mask |= 1 << h
            if name in ("sigma", "alpha"):
                if not (lo > 0 and hi > 0):
                    raise ValueError(f"bounds of {name}: positive")
                lo, hi = np.float32(np.log(lo)), np.float32(np.log(hi))
            c.lo[h], c.hi[h] = lo, hi
        msg = C.c_char_p()
        if check and _ffi.lib().adc_pbt_config_check(C.byref(c), int(members), cls.PBT_KINDS[kind], C.byref(msg)) != _ffi.ADC_OK:
            raise ValueError((msg.value or b"bad PBT configuration").decode())
        return c

    def pbt_init(self, kind, **options):
        """a population-based training scheduler over the live pg_pop ("pg"), td3_pop ("td3") or sac_pop ("sac") trainer; options
        as pbt_config's (members is the learners' count).  It goes when that trainer goes."""
        cfg = self.pbt_config(kind, max(getattr(self, "_learners", 0), 1), check=False, **options)
        init = self._lib.adc_engine_pbt_init_sac if kind == "sac" else self._lib.adc_engine_pbt_init
        check(init(self._h, C.byref(cfg)))
        self._pbt_kind = kind

    def pbt_fitness(self):
        """[M] float64: per member the mean over its envs of the recorded reward summed over the recorded days, reduced on the device"""
        f = np.zeros(max(getattr(self, "_learners", 0), 1), np.float64)
        check(self._lib.adc_engine_pbt_fitness(self._h, f.ctypes.data))
        return f

    def pbt_exploit(self, src_of_member):
        """the batched copy alone: member m becomes a copy of member src_of_member[m] (m itself or -1: kept) in a fixed number of
        launches; no destination may also be a source"""
        src = np.ascontiguousarray(src_of_member, dtype=np.int32)
        if src.shape != (max(getattr(self, "_learners", 0), 1),):
            raise ValueError("pbt_exploit: one source per member")
        check(self._lib.adc_engine_pbt_exploit(self._h, src.ctypes.data))

    def pbt_step(self, fitness=None):
        """one round: fitness (the device's, or `fitness` [M]), smoothing, plan, exploit, explore.  A dict of fitness, smoothed
        [M] float64, rank, src [M] int32 (src -1: kept) and hp [M, 8] float32 (the members' hyperparameters by id after the round; id 4 of "td3" and "sac":
        the log-domain shift the member's log_std / log_alpha got from its donor's before the clamp, 0 when kept)"""
        M = max(getattr(self, "_learners", 0), 1)
        f = None if fitness is None else np.ascontiguousarray(fitness, dtype=np.float64)
        if f is not None and f.shape != (M,):
            raise ValueError("fitness: one value per member")
        res = (_ffi.PBTResult * M)()
        check(self._lib.adc_engine_pbt_step(self._h, None if f is None else f.ctypes.data, res))
        return dict(fitness=np.array([r.fitness for r in res], np.float64), smoothed=np.array([r.smoothed for r in res], np.float64),
                    rank=np.array([r.rank for r in res], np.int32), src=np.array([r.src for r in res], np.int32),
                    hp=np.array([list(r.hp) for r in res], np.float32))

    def pbt_state(self, state=None):
        """get (no argument): dict of round and smoothed [M] float64; set: such a dict - with the trainer's own state the
        scheduler continues bit for bit"""
        M = max(getattr(self, "_learners", 0), 1)
        if state is None:
            r, s = C.c_int64(0), np.zeros(M, np.float64)
            check(self._lib.adc_engine_pbt_state_get(self._h, C.byref(r), s.ctypes.data))
            return dict(round=r.value, smoothed=s)
        s = np.ascontiguousarray(state["smoothed"], dtype=np.float64)
        if s.shape != (M,):
            raise ValueError("pbt_state: one smoothed fitness per member")
        check(self._lib.adc_engine_pbt_state_set(self._h, int(state["round"]), s.ctypes.data))

    # ---- the running observation normaliser fed from the record (parts/kernel_norm.inc; the law is csrc/adc_norm.h) --------------
    @classmethod
    def obs_norm_config(cls, per_member=False, min_std=1e-2, count_cap=0):
        """an adc_obs_norm_config: min_std the floor of the standard deviation; count_cap > 0 bounds the running count (the
        horizon a drifting env needs), 0: off"""
        c = _ffi.ObsNormConfig()
        c.struct_size = C.sizeof(_ffi.ObsNormConfig)
        c.per_member, c.min_std, c.count_cap = 1 if per_member else 0, float(min_std), int(count_cap)
        msg = C.c_char_p()
        if _ffi.lib().adc_obs_norm_config_check(C.byref(c), C.byref(msg)) != _ffi.ADC_OK:
            raise ValueError((msg.value or b"bad observation normaliser configuration").decode())
        return c

    def obs_norm_init(self, **options):
        """a running mean / std filter of the raw observation, starting from the vectors in force (mlp_init with a normalising
        policy first; per_member=True: one per learner, mlp_learners first); options as obs_norm_config's"""
        cfg = self.obs_norm_config(**options)
        check(self._lib.adc_engine_obs_norm_init(self._h, C.byref(cfg)))
        self._obs_norm_members = max(getattr(self, "_learners", 0), 1) if cfg.per_member else 1

    def obs_norm_update(self):
        """merge the recorded days not yet consumed into the running moments and write the new shift / scale where the next
        act reads them (after the trainer's update, before the next rollout_reset)"""
        check(self._lib.adc_engine_obs_norm_update(self._h))

    def obs_norm_state(self, member=0, state=None):
        """one normaliser's state (member 0: the shared one).  get (no state): dict of count, mean, M2 [D] float64, shift, scale
        [D] float32; set: such a dict - with the trainer's own state the run continues bit for bit"""
        D = self.mlp_input_size()
        if state is None:
            st = dict(mean=np.zeros(D, np.float64), M2=np.zeros(D, np.float64), shift=np.zeros(D, np.float32), scale=np.zeros(D, np.float32))
            n = C.c_int64(0)
            check(self._lib.adc_engine_obs_norm_state_get(self._h, int(member), C.byref(n), *(st[k].ctypes.data for k in ("mean", "M2", "shift", "scale"))))
            st["count"] = n.value
            return st
        arr = [np.ascontiguousarray(state[k], dtype=t) for k, t in (("mean", np.float64), ("M2", np.float64), ("shift", np.float32), ("scale", np.float32))]
        if any(a.shape != (D,) for a in arr):
            raise ValueError(f"obs_norm_state: mean, M2, shift and scale have {D} entries")
        check(self._lib.adc_engine_obs_norm_state_set(self._h, int(member), int(state["count"]), *(a.ctypes.data for a in arr)))

    def obs_norm_copy(self, src_of_member):
        """every member's normaliser becomes that of member src_of_member[m] (m itself or -1: kept) in one launch; no
        destination may also be a source (pbt_exploit's convention)"""
        src = np.ascontiguousarray(src_of_member, dtype=np.int32)
        if src.shape != (getattr(self, "_obs_norm_members", 1),):
            raise ValueError("obs_norm_copy: one source per member")
        check(self._lib.adc_engine_obs_norm_copy(self._h, src.ctypes.data))

    # ---- the running reward normaliser fed from the record (parts/kernel_norm.inc; the law is csrc/adc_rew_norm.h) --------------
    @classmethod
    def rew_norm_config(cls, per_member=False, min_std=1e-2, clip=10.0, count_cap=0):
        """an adc_rew_norm_config: min_std the floor of the discounted return's standard deviation; clip > 0 bounds the
        normalised reward to [-clip, clip], 0: off; count_cap > 0 bounds the running count (the horizon a drifting env needs),
        0: off.  The defaults are configuration (VecNormalize's clip), not measurements."""
        c = _ffi.RewNormConfig()
        c.struct_size = C.sizeof(_ffi.RewNormConfig)
        c.per_member, c.min_std, c.clip, c.count_cap = 1 if per_member else 0, float(min_std), float(clip), int(count_cap)
        msg = C.c_char_p()
        if _ffi.lib().adc_rew_norm_config_check(C.byref(c), C.byref(msg)) != _ffi.ADC_OK:
            raise ValueError((msg.value or b"bad reward normaliser configuration").decode())
        return c

    def rew_norm_init(self, **options):
        """a running filter of the discounted return's variance whose reciprocal standard deviation multiplies the reward in
        GAE (pg_init or pg_pop_init first: it discounts by their gamma; per_member=True: one per learner of a population);
        options as rew_norm_config's"""
        cfg = self.rew_norm_config(**options)
        check(self._lib.adc_engine_rew_norm_init(self._h, C.byref(cfg)))
        self._rew_norm_members = max(getattr(self, "_learners", 0), 1) if cfg.per_member else 1

    def rew_norm_update(self):
        """merge the recorded days not yet consumed into the running moments and write the new multiplier where the next
        advantages call reads it (before the trainer's update)"""
        check(self._lib.adc_engine_rew_norm_update(self._h))

    def rew_norm_state(self, member=0, state=None):
        """one normaliser's state (member 0: the shared one).  get (no state): dict of count, mean, M2 (float64), scale
        (float32); set: such a dict - with rew_norm_returns and the trainer's own state the run continues bit for bit"""
        if state is None:
            n, mean, m2, sc = C.c_int64(0), C.c_double(0.0), C.c_double(0.0), C.c_float(0.0)
            check(self._lib.adc_engine_rew_norm_state_get(self._h, int(member), C.byref(n), C.byref(mean), C.byref(m2), C.byref(sc)))
            return dict(count=n.value, mean=np.float64(mean.value), M2=np.float64(m2.value), scale=np.float32(sc.value))
        check(self._lib.adc_engine_rew_norm_state_set(self._h, int(member), int(state["count"]), float(state["mean"]), float(state["M2"]),
                                                      float(np.float32(state["scale"]))))

    def rew_norm_returns(self, values=None):
        """the envs' running discounted returns [N] float64 (the scan's carry).  get (no argument) or set"""
        if values is None:
            g = np.zeros(self.num_envs, np.float64)
            check(self._lib.adc_engine_rew_norm_returns_get(self._h, g.ctypes.data))
            return g
        g = np.ascontiguousarray(values, dtype=np.float64)
        if g.shape != (self.num_envs,):
            raise ValueError("rew_norm_returns: one value per env")
        check(self._lib.adc_engine_rew_norm_returns_set(self._h, g.ctypes.data))

    def rew_norm_copy(self, src_of_member):
        """every member's reward normaliser becomes that of member src_of_member[m] (m itself or -1: kept) in one launch; no
        destination may also be a source (pbt_exploit's convention).  The envs' running returns stay."""
        src = np.ascontiguousarray(src_of_member, dtype=np.int32)
        if src.shape != (getattr(self, "_rew_norm_members", 1),):
            raise ValueError("rew_norm_copy: one source per member")
        check(self._lib.adc_engine_rew_norm_copy(self._h, src.ctypes.data))

    # ---- the TD3 learners' running normalisers (parts/kernel_norm.inc; the law is csrc/adc_td3_norm.h) ----------------------------
    @classmethod
    def td3_norm_config(cls, observations=False, rewards=False, per_member=False, obs_min_std=1e-2, obs_count_cap=0, rew_min_std=1e-2, rew_count_cap=0,
                        rew_clip=10.0):
        """an adc_td3_norm_config: which parts live (at least one); the min_std floor the standard deviations; the count_cap > 0
        bound the running counts, 0: off; rew_clip > 0 bounds the normalised reward, 0: off.  The defaults are configuration
        (VecNormalize's clip), not measurements."""
        c = _ffi.TD3NormConfig()
        c.struct_size = C.sizeof(_ffi.TD3NormConfig)
        c.observations, c.rewards, c.per_member = 1 if observations else 0, 1 if rewards else 0, 1 if per_member else 0
        c.obs_min_std, c.obs_count_cap, c.rew_min_std, c.rew_count_cap, c.rew_clip = float(obs_min_std), int(obs_count_cap), float(rew_min_std), int(rew_count_cap), float(rew_clip)
        msg = C.c_char_p()
        if _ffi.lib().adc_td3_norm_config_check(C.byref(c), C.byref(msg)) != _ffi.ADC_OK:
            raise ValueError((msg.value or b"bad TD3 normaliser configuration").decode())
        return c

    def td3_norm_init(self, **options):
        """running normalisers for the live TD3 trainer (td3_init or td3_pop_init first, the record and the ring still empty):
        with observations the record and the ring hold RAW observations from here on and every batch is normalised as it is
        sampled; with rewards the target's reward is multiplied by the reciprocal running standard deviation of the discounted
        return.  per_member=True: one per learner of a population.  Options as td3_norm_config's"""
        cfg = self.td3_norm_config(**options)
        check(self._lib.adc_engine_td3_norm_init(self._h, C.byref(cfg)))
        self._td3_norm = dict(members=max(getattr(self, "_learners", 0), 1) if cfg.per_member else 1, observations=bool(cfg.observations),
                              rewards=bool(cfg.rewards))

    def _ring_norm_info(self, family):
        """what {family}_norm_init set up; without one the engine itself says what is missing"""
        info = getattr(self, f"_{family}_norm", None)
        if info is None:
            check(getattr(self._lib, f"adc_engine_{family}_norm_state_get")(self._h, 0, *([None] * 9)))
            info = dict(members=1, observations=True, rewards=True)
        return info

    def _ring_norm_update(self, family):
        n = C.c_int64(0)
        check(getattr(self._lib, f"adc_engine_{family}_norm_update")(self._h, C.byref(n)))
        return n.value

    def _ring_norm_state(self, family, member, state):
        """the state of one normaliser of an off-policy family (td3 / sac): the two families share the entry points' signatures"""
        D, info = self.mlp_input_size(), self._ring_norm_info(family)
        okeys = (("obs_mean", np.float64), ("obs_M2", np.float64), ("shift", np.float32), ("scale", np.float32))
        if state is None:
            st = {}
            optr = [None] * 4
            n, rn, mean, m2, sc = C.c_int64(0), C.c_int64(0), C.c_double(0.0), C.c_double(0.0), C.c_float(0.0)
            if info["observations"]:
                st.update({k: np.zeros(D, t) for k, t in okeys})
                optr = [st[k].ctypes.data for k, _ in okeys]
            rptr = [C.byref(rn), C.byref(mean), C.byref(m2), C.byref(sc)] if info["rewards"] else [None] * 4
            check(getattr(self._lib, f"adc_engine_{family}_norm_state_get")(self._h, int(member), C.byref(n) if info["observations"] else None, *optr, *rptr))
            if info["observations"]:
                st["obs_count"] = n.value
            if info["rewards"]:
                st.update(rew_count=rn.value, rew_mean=np.float64(mean.value), rew_M2=np.float64(m2.value), rew_scale=np.float32(sc.value))
            return st
        arr = [None] * 4
        if info["observations"]:
            arr = [np.ascontiguousarray(state[k], dtype=t) for k, t in okeys]
            if any(a.shape != (D,) for a in arr):
                raise ValueError(f"{family}_norm_state: obs_mean, obs_M2, shift and scale have {D} entries")
        rew = (int(state["rew_count"]), float(state["rew_mean"]), float(state["rew_M2"]), float(np.float32(state["rew_scale"]))) if info["rewards"] else (0, 0.0, 0.0, 1.0)
        check(getattr(self._lib, f"adc_engine_{family}_norm_state_set")(self._h, int(member), int(state["obs_count"]) if info["observations"] else 0,
                                                                        *(None if a is None else a.ctypes.data for a in arr), *rew))

    def _ring_norm_returns(self, family, values):
        if values is None:
            g = np.zeros(self.num_envs, np.float64)
            check(getattr(self._lib, f"adc_engine_{family}_norm_returns_get")(self._h, g.ctypes.data))
            return g
        g = np.ascontiguousarray(values, dtype=np.float64)
        if g.shape != (self.num_envs,):
            raise ValueError(f"{family}_norm_returns: one value per env")
        check(getattr(self._lib, f"adc_engine_{family}_norm_returns_set")(self._h, g.ctypes.data))

    def _ring_norm_copy(self, family, src_of_member):
        src = np.ascontiguousarray(src_of_member, dtype=np.int32)
        if src.shape != (self._ring_norm_info(family)["members"],):
            raise ValueError(f"{family}_norm_copy: one source per member")
        check(getattr(self._lib, f"adc_engine_{family}_norm_copy")(self._h, src.ctypes.data))

    def _td3_norm_info(self):
        """what td3_norm_init set up; without one the engine itself says what is missing"""
        return self._ring_norm_info("td3")

    def td3_norm_update(self):
        """merge the recorded days not yet consumed into the running moments and write the new vectors and multiplier where the
        next act and the next td3_update read them (after the store, before the updates); returns the samples consumed"""
        return self._ring_norm_update("td3")

    def td3_norm_state(self, member=0, state=None):
        """one normaliser's state (member 0: the shared one).  get (no state): dict of the living parts - obs_count, obs_mean,
        obs_M2 [D] float64, shift, scale [D] float32; rew_count, rew_mean, rew_M2 (float64), rew_scale (float32); set: such a dict -
        with td3_norm_returns, the trainer's state and the ring the run continues bit for bit"""
        return self._ring_norm_state("td3", member, state)

    def td3_norm_returns(self, values=None):
        """the envs' running discounted returns [N] float64 (the reward part's carry).  get (no argument) or set"""
        return self._ring_norm_returns("td3", values)

    def td3_norm_copy(self, src_of_member):
        """every member's normalisers become those of member src_of_member[m] (m itself or -1: kept) in one launch; no
        destination may also be a source (pbt_exploit's convention).  The envs' running returns stay."""
        self._ring_norm_copy("td3", src_of_member)

    # ---- the SAC learners' running normalisers (parts/kernel_norm.inc; the law is csrc/adc_sac_norm.h) ----------------------------
    @classmethod
    def sac_norm_config(cls, observations=False, rewards=False, per_member=False, obs_min_std=1e-2, obs_count_cap=0, rew_min_std=1e-2, rew_count_cap=0,
                        rew_clip=10.0):
        """an adc_sac_norm_config: td3_norm_config's fields and defaults (configuration, not measurements)"""
        c = _ffi.SACNormConfig()
        c.struct_size = C.sizeof(_ffi.SACNormConfig)
        c.observations, c.rewards, c.per_member = 1 if observations else 0, 1 if rewards else 0, 1 if per_member else 0
        c.obs_min_std, c.obs_count_cap, c.rew_min_std, c.rew_count_cap, c.rew_clip = float(obs_min_std), int(obs_count_cap), float(rew_min_std), int(rew_count_cap), float(rew_clip)
        msg = C.c_char_p()
        if _ffi.lib().adc_sac_norm_config_check(C.byref(c), C.byref(msg)) != _ffi.ADC_OK:
            raise ValueError((msg.value or b"bad SAC normaliser configuration").decode())
        return c

    def sac_norm_init(self, **options):
        """running normalisers for the live SAC trainer (sac_init or sac_pop_init first, the record and the ring still empty): with
        observations the record and the ring hold RAW observations from here on and every batch is normalised as it is sampled;
        with rewards the target's reward is multiplied by the reciprocal running standard deviation of the discounted return - the
        entropy term is not, so target_entropy / alpha then trade against a return of about unit scale.  per_member=True: one per
        learner of a population.  Options as sac_norm_config's"""
        cfg = self.sac_norm_config(**options)
        check(self._lib.adc_engine_sac_norm_init(self._h, C.byref(cfg)))
        self._sac_norm = dict(members=max(getattr(self, "_learners", 0), 1) if cfg.per_member else 1, observations=bool(cfg.observations),
                              rewards=bool(cfg.rewards))

    def sac_norm_update(self):
        """merge the recorded days not yet consumed into the running moments and write the new vectors and multiplier where the
        next act and the next sac_update read them (after the store, before the updates); returns the samples consumed"""
        return self._ring_norm_update("sac")

    def sac_norm_state(self, member=0, state=None):
        """one normaliser's state, get or set: td3_norm_state's dict"""
        return self._ring_norm_state("sac", member, state)

    def sac_norm_returns(self, values=None):
        """the envs' running discounted returns [N] float64 (the reward part's carry).  get (no argument) or set"""
        return self._ring_norm_returns("sac", values)

    def sac_norm_copy(self, src_of_member):
        """every member's normalisers become those of member src_of_member[m] (m itself or -1: kept) in one launch; no
        destination may also be a source (pbt_exploit's convention).  The envs' running returns stay."""
        self._ring_norm_copy("sac", src_of_member)

    # ---- prioritised replay for the TD3 / SAC learners (parts/kernel_per.inc; the law is csrc/adc_per.h) -------------------------
    @classmethod
    def replay_prio_config(cls, alpha=0.6, beta=0.4, eps=1e-6, cap=1e6):
        """an adc_replay_prio_config: alpha in [0, 1] the priorities' exponent, beta in [0, 1] the importance weights', eps > 0
        added to the error (and the floor of a priority), cap > eps its ceiling.  The defaults are the usual configuration
        (Schaul et al. 2016), not measurements."""
        c = _ffi.ReplayPrioConfig()
        c.struct_size = C.sizeof(_ffi.ReplayPrioConfig)
        c.alpha, c.beta, c.eps, c.cap = float(alpha), float(beta), float(eps), float(cap)
        msg = C.c_char_p()
        if _ffi.lib().adc_replay_prio_config_check(C.byref(c), C.byref(msg)) != _ffi.ADC_OK:
            raise ValueError((msg.value or b"bad prioritised replay configuration").decode())
        return c

    def replay_prio_init(self, **options):
        """prioritised replay for the live TD3 / SAC trainer, solo or population (td3_init, sac_init, td3_pop_init or sac_pop_init
        first): batches are drawn from a sum tree on the device in proportion to the slots' priorities, the critics' loss is
        weighted by the importance weights, the priorities follow the critics' errors.  A ring that already holds transitions is
        fine (its slots get leaf 1).  Options as replay_prio_config's; it ends with its trainer"""
        cfg = self.replay_prio_config(**options)
        check(self._lib.adc_engine_replay_prio_init(self._h, C.byref(cfg)))

    def replay_prio_set_beta(self, beta):
        """the importance weights' exponent from the next update on (the host's annealing schedule)"""
        check(self._lib.adc_engine_replay_prio_set_beta(self._h, float(beta)))

    def replay_prio_info(self, member=0):
        """dict of total (the tree's root, float64) and top (the largest leaf any update has written, float32)"""
        total, top = C.c_double(0.0), C.c_float(0.0)
        check(self._lib.adc_engine_replay_prio_info(self._h, int(member), C.byref(total), C.byref(top)))
        return dict(total=np.float64(total.value), top=np.float32(top.value))

    def _replay_prio_sizes(self):
        """(ring size, batch size) of whichever off-policy trainer lives; without one the engine itself says what is missing"""
        L, h, b, sz = self._lib, self._h, C.c_int32(0), C.c_int64(0)
        if L.adc_engine_td3_batch_size(h, C.byref(b)) == _ffi.ADC_OK:
            check(L.adc_engine_td3_buffer_info(h, C.byref(sz), None, None))
        elif L.adc_engine_sac_batch_size(h, C.byref(b)) == _ffi.ADC_OK:
            check(L.adc_engine_sac_buffer_info(h, C.byref(sz), None, None))
        elif L.adc_engine_td3_pop_buffer_info(h, C.byref(sz), None, None, C.byref(b)) != _ffi.ADC_OK:
            if L.adc_engine_sac_pop_buffer_info(h, C.byref(sz), None, None, C.byref(b)) != _ffi.ADC_OK:
                check(L.adc_engine_replay_prio_info(h, 0, None, None))
                raise RuntimeError("prioritised replay without an off-policy trainer")
        return sz.value, b.value

    def replay_prio_fetch(self, member=0, slot=0, count=None):
        """the leaves of the slots [slot, slot + count) (default: up to the ring's size): float32"""
        if count is None:
            count = self._replay_prio_sizes()[0] - int(slot)
        leaf = np.zeros(max(int(count), 0), np.float32)
        if leaf.size or count != 0:
            check(self._lib.adc_engine_replay_prio_fetch(self._h, int(member), int(slot), int(count), leaf.ctypes.data))
        return leaf

    def replay_prio_load(self, leaf, top, member=0, slot=0):
        """leaves (finite, > 0) for the stored slots from `slot` on, and top; the tree's nodes are rebuilt"""
        leaf = np.ascontiguousarray(leaf, dtype=np.float32)
        if leaf.ndim != 1:
            raise ValueError("replay_prio_load: leaf [count]")
        check(self._lib.adc_engine_replay_prio_load(self._h, int(member), int(slot), leaf.size, leaf.ctypes.data, float(np.float32(top))))

    def replay_prio_batch(self, update, member=0):
        """what update number `update` would draw from the tree as it stands: (slots [batch_size] int32, weights [batch_size] float32)"""
        B = self._replay_prio_sizes()[1]
        idx, w = np.zeros(B, np.int32), np.zeros(B, np.float32)
        check(self._lib.adc_engine_replay_prio_batch(self._h, int(member), int(update), idx.ctypes.data, w.ctypes.data))
        return idx, w

    def replay_prio_state(self, member=0, state=None):
        """a member's priorities.  get (no state): dict of leaf [size] float32 and top; set: such a dict, after the ring was loaded -
        with the trainer's state and the ring the run continues bit for bit"""
        if state is None:
            size = self._replay_prio_sizes()[0]
            return dict(leaf=self.replay_prio_fetch(member, 0, size) if size else np.zeros(0, np.float32), top=self.replay_prio_info(member)["top"])
        if np.asarray(state["leaf"]).size:
            self.replay_prio_load(state["leaf"], state["top"], member)

    # ---- n-step returns for the TD3 / SAC learners (parts/nstep_api.inc; the law is csrc/adc_td3.h "n-step") ------------------------
    def replay_nstep_init(self, n):
        """n-step returns for the live TD3 / SAC trainer, solo or population (td3_init, sac_init, td3_pop_init or sac_pop_init first):
        from the next store on a slot holds the discounted sum of up to n days' rewards, the last summed day's done flag, the
        observation after them and its own bootstrap discount gn, which the targets read in gamma's place.  Windows are cut at an
        episode's end and at the end of the stored days.  n in 1..16, shared by a population's members; a ring that already holds
        transitions is fine (its slots get gn = gamma); a second call changes the window.  It ends with its trainer"""
        check(self._lib.adc_engine_replay_nstep_init(self._h, int(n)))

    def replay_nstep_info(self):
        """the window n, 0 while the add-on is off"""
        n = C.c_int32(0)
        check(self._lib.adc_engine_replay_nstep_info(self._h, C.byref(n)))
        return int(n.value)

    def replay_nstep_fetch(self, member=0, slot=0, count=None):
        """the bootstrap discounts gn of the slots [slot, slot + count) (default: up to the ring's size): float32"""
        if count is None:
            if self.replay_nstep_info() == 0:           # (the engine's own words for what is missing)
                check(self._lib.adc_engine_replay_nstep_fetch(self._h, int(member), 0, 1, None))
            count = self._replay_prio_sizes()[0] - int(slot)
        gn = np.zeros(max(int(count), 0), np.float32)
        if gn.size or count != 0:
            check(self._lib.adc_engine_replay_nstep_fetch(self._h, int(member), int(slot), int(count), gn.ctypes.data))
        return gn

    def replay_nstep_load(self, gn, member=0, slot=0):
        """bootstrap discounts (finite, >= 0) for the slots from `slot` on, next to *_buffer_load, which moves R and done"""
        gn = np.ascontiguousarray(gn, dtype=np.float32)
        if gn.ndim != 1:
            raise ValueError("replay_nstep_load: gn [count]")
        check(self._lib.adc_engine_replay_nstep_load(self._h, int(member), int(slot), gn.size, gn.ctypes.data))

    def replay_nstep_state(self, member=0, state=None):
        """a member's n-step side of the ring.  get (no state): dict of n and gn [size] float32; set: such a dict, after the ring was
        loaded - with the trainer's state and the ring the run continues bit for bit"""
        if state is None:
            size = self._replay_prio_sizes()[0]
            return dict(n=self.replay_nstep_info(), gn=self.replay_nstep_fetch(member, 0, size) if size else np.zeros(0, np.float32))
        if int(state["n"]) != self.replay_nstep_info():
            self.replay_nstep_init(int(state["n"]))
        if np.asarray(state["gn"]).size:
            self.replay_nstep_load(state["gn"], member)

    def rollout_enable(self, horizon, obs=False):
        check(self._lib.adc_engine_rollout_enable(self._h, int(horizon), 1 if obs else 0))
        self._td3_norm = self._sac_norm = None                   # (the TD3 normalisers, if any, ended with their trainer)
        self._rollout_obs = bool(obs) and int(horizon) > 0

    def rollout_reset(self):
        check(self._lib.adc_engine_rollout_reset(self._h))

    def rollout_fetch(self, bootstrap=False):
        """the recorded days so far: dict of action [T, N, K+1], logp, value, reward [T, N] (float32), terminated, truncated
        [T, N] (bool), obs [T, N, D] when recorded; bootstrap=True adds bootstrap_value [N]"""
        t = C.c_int32(0)
        check(self._lib.adc_engine_rollout_fetch(self._h, C.byref(t), *([None] * 7)))
        T, n, a = t.value, self.num_envs, self.num_keywords + 1
        st = dict(action=np.zeros((T, n, a), np.float32), logp=np.zeros((T, n), np.float32), value=np.zeros((T, n), np.float32),
                  reward=np.zeros((T, n), np.float32), terminated=np.zeros((T, n), np.uint8), truncated=np.zeros((T, n), np.uint8))
        if getattr(self, "_rollout_obs", False):
            st["obs"] = np.zeros((T, n, self.mlp_input_size()), np.float32)
        check(self._lib.adc_engine_rollout_fetch(self._h, None, *(st[k].ctypes.data for k in (
            "action", "logp", "value", "reward", "terminated", "truncated")), st["obs"].ctypes.data if "obs" in st else None))
        st["terminated"], st["truncated"] = st["terminated"].astype(bool), st["truncated"].astype(bool)
        if bootstrap:
            st["bootstrap_value"] = self.mlp_bootstrap_value()
        return st

    POLICIES = {"fixed": 0, "zero_margin": 1, "oracle": 2, "interpolation": 3, "mlp": 4}

    # ---- multi-GPU: the episode-metric all-reduce (RCCL behind the C ABI; adcraft_amd/comm.py brings it up) ----------
    def comm_unique_id(self):
        buf = (C.c_uint8 * 128)()
        check(self._lib.adc_comm_get_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id, rank, world_size):
        uid = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        check(self._lib.adc_engine_comm_init(self._h, uid, int(rank), int(world_size)))

    def comm_destroy(self):
        check(self._lib.adc_engine_comm_destroy(self._h))

    def comm_info(self):
        r, w = C.c_int32(0), C.c_int32(1)
        check(self._lib.adc_engine_comm_info(self._h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def comm_stats(self, reset=False):
        """(calls, ms of this rank's own reduction kernels, ms of the ncclAllReduce) of the metric reductions so far"""
        n, a, b = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
        check(self._lib.adc_engine_comm_stats(self._h, C.byref(n), C.byref(a), C.byref(b), 1 if reset else 0))
        return n.value, a.value, b.value

    def region_begin(self):
        """one event on the engine's stream; region_end() -> GPU milliseconds since (one event pair for a whole timed region)"""
        check(self._lib.adc_engine_region_begin(self._h))

    def region_end(self):
        ms = C.c_double(0.0)
        check(self._lib.adc_engine_region_end(self._h, C.byref(ms)))
        return ms.value

    def metrics_allreduce(self, ideal_k=None, ideal_pos_k=None):
        """the one collective of the path: (profit_cents[K], ideal[K], ideal_pos[K], scalars[8]) summed over steps, envs and
        the ranks of the engine's communicator (this rank alone without one)"""
        K = self.num_keywords
        out = np.zeros(3 * K + 8, dtype=np.float64)
        a = None if ideal_k is None else np.ascontiguousarray(ideal_k, dtype=np.float64)
        b = None if ideal_pos_k is None else np.ascontiguousarray(ideal_pos_k, dtype=np.float64)
        check(self._lib.adc_engine_metrics_allreduce(self._h, None if a is None else a.ctypes.data,
                                                     None if b is None else b.ctypes.data, out.ctypes.data))
        return out[:K], out[K:2 * K], out[2 * K:3 * K], out[3 * K:]

    def comm_allreduce(self, values, op="sum"):
        v = np.ascontiguousarray(values, dtype=np.float64).copy()
        check(self._lib.adc_engine_comm_allreduce_f64(self._h, v.ctypes.data, v.size, 1 if op == "max" else 0))
        return v

    def run_days(self, policy, days, budget=100000.0, graph=None):
        """`days` days of the device-resident loop in one call; graph=True replays pairs of days from a captured
        hipGraph (same results, measured no faster: tools/experiments/measure_small_loop.py)"""
        if graph is not None:
            check(self._lib.adc_engine_day_graph_enable(self._h, 1 if graph else 0))
        check(self._lib.adc_engine_run_days(self._h, self.POLICIES[policy], int(days), float(budget)))

    # ---- imitation learning: teacher days, behaviour cloning and MARWIL (parts/imitation_api.inc; the law is csrc/adc_imitation.h) ----
    def teach_days(self, teacher, days, budget=100000.0):
        """`days` teacher days: the learned agent acts (its action thrown away, its input row and value recorded), `teacher` -
        "fixed", "zero_margin", "oracle" or "interpolation" - acts as run_days has it act, the record keeps the teacher's action
        (logp +0), the env steps.  Needs mlp_init and rollout_enable(T, obs=True); the env ends where run_days(teacher) leaves it."""
        if teacher not in self.POLICIES:
            raise ValueError(f"unknown teacher {teacher!r}: one of {sorted(self.POLICIES)}")
        check(self._lib.adc_engine_teach_days(self._h, self.POLICIES[teacher], int(days), float(budget)))

    def dagger_days(self, teacher, days, beta, budget=100000.0):
        """`days` DAgger days (csrc/adc_dagger.h): learner and teacher act on the same observation as on a teacher day, the record
        keeps the teacher's action as the label (logp +0), and a per-env coin - the teacher with probability `beta` - picks whose
        action the step consumes.  beta 1 is teach_days bit for bit, beta 0 the learner's own day with the teacher's label.
        `teacher`: "fixed", "zero_margin" or "oracle".  get_actions() afterwards returns the label; dagger_mask() who drove."""
        if teacher not in self.POLICIES:
            raise ValueError(f"unknown teacher {teacher!r}: one of {sorted(self.POLICIES)}")
        check(self._lib.adc_engine_dagger_days(self._h, self.POLICIES[teacher], int(days), float(budget), float(beta)))

    def dagger_mask(self):
        """uint8 [T_recorded, N]: 1 where the teacher's action was the one the step consumed (rows of plain teacher days read 1)"""
        t = C.c_int32(0)
        check(self._lib.adc_engine_rollout_fetch(self._h, C.byref(t), *([None] * 7)))
        out = np.zeros((t.value, self.num_envs), np.uint8)
        buf = out if out.size else np.zeros(1, np.uint8)         # (an empty record: still a valid pointer)
        check(self._lib.adc_engine_dagger_mask_fetch(self._h, buf.ctypes.data))
        return out

    @classmethod
    def im_config(cls, beta=0.0, vf_coef=1.0, w_max=20.0, ma_start=100.0, ma_rate=1e-8, train_log_std=True):
        """an adc_im_config: beta 0 is behaviour cloning (w = 1), beta > 0 MARWIL's exp(beta adv / c) capped at w_max (0: no cap);
        vf_coef 0 drops the value loss; ma_start / ma_rate: the moving scale of the advantages (RLlib's 100 and 1e-8);
        train_log_std False leaves the free log_std as it is (the user's action scale)"""
        c = _ffi.IMConfig()
        c.struct_size = C.sizeof(_ffi.IMConfig)
        c.beta, c.vf_coef, c.w_max, c.ma_start, c.ma_rate = float(beta), float(vf_coef), float(w_max), float(ma_start), float(ma_rate)
        c.train_log_std = 1 if train_log_std else 0
        msg = C.c_char_p()
        if _ffi.lib().adc_im_config_check(C.byref(c), C.byref(msg)) != _ffi.ADC_OK:
            raise ValueError((msg.value or b"bad imitation configuration").decode())
        return c

    def im_init(self, **options):
        """imitation over the live single-learner trainer (pg_init first): it trains that trainer's theta with its optimiser; options
        as im_config's"""
        cfg = self.im_config(**options)
        check(self._lib.adc_engine_im_init(self._h, C.byref(cfg)))

    def im_advantages(self, fetch=False):
        """the teacher's discounted returns over the recorded teacher days and the moving scale's update; fetch=True returns
        (adv, ret) [T, N] float32"""
        if not fetch:
            check(self._lib.adc_engine_im_advantages(self._h, None, None))
            return None
        t = C.c_int32(0)
        check(self._lib.adc_engine_rollout_fetch(self._h, C.byref(t), *([None] * 7)))
        adv, ret = np.zeros((t.value, self.num_envs), np.float32), np.zeros((t.value, self.num_envs), np.float32)
        check(self._lib.adc_engine_im_advantages(self._h, adv.ctypes.data, ret.ctypes.data))
        return adv, ret

    @staticmethod
    def _im_stats(st):
        return {k: getattr(st, k) for k, _ in _ffi.IMStats._fields_}

    def im_minibatch(self, env_begin, env_count):
        """one gradient of the imitation loss and one optimiser step over every recorded day of the envs [env_begin, env_begin + env_count)"""
        st = _ffi.IMStats()
        check(self._lib.adc_engine_im_minibatch(self._h, int(env_begin), int(env_count), C.byref(st)))
        return self._im_stats(st)

    def im_update(self, epochs=1):
        """`epochs` x the minibatches of minibatch_envs in ascending env order (im_advantages first); the last epoch's statistics"""
        st = _ffi.IMStats()
        check(self._lib.adc_engine_im_update(self._h, int(epochs), C.byref(st)))
        return self._im_stats(st)

    def im_state(self, state=None):
        """get (no argument): dict of ma and calls; set: such a dict (theta, m, v and steps are pg_state's)"""
        if state is None:
            ma, calls = C.c_double(0.0), C.c_int64(0)
            check(self._lib.adc_engine_im_state_get(self._h, C.byref(ma), C.byref(calls)))
            return dict(ma=ma.value, calls=calls.value)
        check(self._lib.adc_engine_im_state_set(self._h, float(state["ma"]), int(state["calls"])))

    def metrics_akncp_ncp(self, days):
        """(AKNCP [N], NCP [N]) of the running episode, reduced on the device (per-env median over the keywords in LDS)"""
        a, b = np.zeros(self.num_envs, np.float64), np.zeros(self.num_envs, np.float64)
        check(self._lib.adc_engine_metrics_akncp_ncp(self._h, float(days), a.ctypes.data, b.ctypes.data))
        return a, b

    def metrics_read_nk(self, ideal=True):
        """per (env, keyword) sums: profit in dollars, and (if ideal) the ideal sum and the ideal sum with <= 0 -> 1"""
        shape = (self.num_envs, self.num_keywords)
        pc = np.zeros(shape, np.int64)
        si = np.zeros(shape, np.float64) if ideal else None
        sp = np.zeros(shape, np.float64) if ideal else None
        check(self._lib.adc_engine_metrics_read_nk(self._h, pc.ctypes.data, None if si is None else si.ctypes.data,
                                                   None if sp is None else sp.ctypes.data))
        return pc / 100.0, si, sp


class ShardedStepEngine:
    """One vector of envs on ONE device, held by several engines (each with its own HIP stream) and stepped together.

    A host-in / host-out step is PCIe-bound (4 B per keyword up, 20 B down, against a 0.2 ms kernel at 4096 x 256): with the
    envs split over a few engines, enqueued asynchronously from page-locked buffers (adc_engine_step_async), one part's
    transfers overlap another part's kernels.  Results are those of a single engine: random streams are keyed by the
    GLOBAL env id (the multi-GPU sharding invariant).  The I/O arrays are single [N, K] page-locked arrays; every part reads
    and writes its rows of them, so callers see the same buffers a StepEngine gives them."""

    def __init__(self, num_envs, num_keywords, model=MODEL_IMPLICIT, *, shards=4, env_id_base=0, compact_counts=False, **kw):
        self.num_envs, self.num_keywords, self.model = int(num_envs), int(num_keywords), int(model)
        if np.ndim(shards):          # relative sizes: a small first part puts its results on the bus early
            edges = np.concatenate([[0.0], np.cumsum(np.asarray(shards, dtype=np.float64))])
            self.bounds = sorted(set(int(round(b)) for b in edges / edges[-1] * self.num_envs))
        else:
            shards = max(1, min(int(shards), self.num_envs))
            self.bounds = [int(b) for b in np.linspace(0, self.num_envs, shards + 1)]
        self.parts = [StepEngine(b1 - b0, num_keywords, model, env_id_base=env_id_base + b0, **kw)
                      for b0, b1 in zip(self.bounds[:-1], self.bounds[1:])]
        N, K = self.num_envs, self.num_keywords
        alloc = self.parts[0]._pinned_array
        self.compact_counts = bool(compact_counts)
        # per-keyword outputs: planes of one [., N, K] page-locked array (a part's rows of all planes = one 2-D transfer);
        # per-env outputs: every part has its own small block laid out like its device block (one transfer), gathered into
        # the [N] arrays after the wait
        per_kw = [n for n, _, k in _OUT_SPEC if k and not (self.compact_counts and n in _COUNT_NAMES)]
        planes = alloc((len(per_kw), N, K), np.int32)
        self.out = {n: planes[i].view(dict((a, b) for a, b, _ in _OUT_SPEC)[n]) for i, n in enumerate(per_kw)}
        self._counts_u16, self._overflow = None, None
        if self.compact_counts:
            self._counts_u16, self._overflow = alloc((N, 3, K), np.uint16), alloc((len(self.parts),), np.int32)
            for i, n in enumerate(_COUNT_NAMES):
                self.out[n] = self._counts_u16[:, i, :]
        per_env = [n for n, _, k in _OUT_SPEC if not k]
        self.out.update({n: np.zeros(N, dt) for n, dt, k in _OUT_SPEC if not k})
        self._small = []
        for p in self.parts:
            off, total = _out_offsets(p._lib, p._h)
            self._small.append(_views_at(alloc((total - off[5],), np.uint8), [o - off[5] for o in off], p.num_envs, K, per_env))
        self._bids_stage, self._budget_stage = alloc((N, K), np.float32), alloc((N,), np.float32)
        self._flat_act, self._flat_obs = None, None
        self._in_ptrs = [(self._bids_stage[b0:b1].ctypes.data, self._budget_stage[b0:b1].ctypes.data)
                         for b0, b1 in zip(self.bounds[:-1], self.bounds[1:])]
        self._outs = []
        for i, (b0, b1) in enumerate(zip(self.bounds[:-1], self.bounds[1:])):
            o = _out_struct(self.out, self._counts_u16, self._overflow, b0, b1, self._small[i])
            if self._overflow is not None:
                o.counts_overflow = self._overflow[i:i + 1].ctypes.data
            self._outs.append(o)

    def _each(self):
        return zip(self.parts, self.bounds[:-1], self.bounds[1:])

    def __getattr__(self, name):
        # (only reached for names this class does not define: the device-resident agent / metric / curve calls of StepEngine)
        if hasattr(StepEngine, name):
            raise NotImplementedError(f"{name}() works on one engine: construct the env / engine with engine_shards=1 "
                                      "(several engines per device only serve the host-in / host-out step)")
        raise AttributeError(name)

    def close(self):
        self.out, self._bids_stage, self._budget_stage, self._flat_act, self._flat_obs = {}, None, None, None, None
        self._counts_u16, self._overflow, self._small = None, None, []
        for p in self.parts:
            p.close()
        self.parts = []

    def set_all_params(self, planes):
        for p, b0, b1 in self._each():
            p.set_all_params(np.ascontiguousarray(planes[:, b0:b1]))

    def get_all_params(self):
        return np.concatenate([p.get_all_params() for p in self.parts], axis=1)

    def reset(self, env_mask=None, seeds=None):
        for p, b0, b1 in self._each():
            p.reset(None if env_mask is None else np.asarray(env_mask)[b0:b1], None if seeds is None else np.asarray(seeds)[b0:b1])

    def generate_keywords(self, table, no_vol_prob=0.0, env_mask=None, serial=0):
        for p, b0, b1 in self._each():
            p.generate_keywords(table, no_vol_prob, None if env_mask is None else np.asarray(env_mask)[b0:b1], serial)

    def generate_explicit_keywords(self, env_mask=None, serial=0):
        for p, b0, b1 in self._each():
            p.generate_explicit_keywords(None if env_mask is None else np.asarray(env_mask)[b0:b1], serial)

    def set_limits(self, max_days, loss_threshold):
        for p in self.parts:
            p.set_limits(max_days, loss_threshold)

    def set_drift(self, enabled, drift=(0.03, 0.03, 0.03)):
        for p in self.parts:
            p.set_drift(enabled, drift)

    def set_drift_mask(self, mask):
        m = None if mask is None else np.asarray(mask)
        for p, b0, b1 in self._each():
            p.set_drift_mask(None if m is None else m if m.ndim == 1 else m[b0:b1])

    def set_env_drift(self, rates):
        r = None if rates is None else np.asarray(rates, dtype=np.float32)
        for p, b0, b1 in self._each():
            p.set_env_drift(None if r is None else r if r.ndim == 1 else r[b0:b1])

    def get_rng_state(self):
        ks, ts = zip(*(p.get_rng_state() for p in self.parts))
        return np.concatenate(ks), np.concatenate(ts)

    def synchronize(self):
        for p in self.parts:
            p.synchronize()

    def step(self, bids, budget, copy=True):
        """host in / host out: every part's step is enqueued, then all are awaited"""
        stage_bids = not _is_buffer(bids, self._bids_stage)      # action_buffers() filled in place: nothing to stage
        if stage_bids and np.ndim(bids):
            bids = np.asarray(bids, dtype=np.float32).reshape(-1, self.num_keywords)
        if not _is_buffer(budget, self._budget_stage):
            self._budget_stage[...] = budget
        for (p, b0, b1), o, (pb, pg) in zip(self._each(), self._outs, self._in_ptrs):
            if stage_bids:                              # part by part: the next part is staged while this one's transfer runs
                self._bids_stage[b0:b1] = bids[b0:b1] if np.ndim(bids) else bids
            p.step_async(pb, pg, o)
        self._wait_and_gather()
        _check_overflow(self._overflow)
        return {k: v.copy() for k, v in self.out.items()} if copy else self.out

    def _wait_and_gather(self):
        for p in self.parts:
            p.wait()
        for small, b0, b1 in zip(self._small, self.bounds[:-1], self.bounds[1:]):
            for name, a in small.items():
                self.out[name][b0:b1] = a

    def action_buffers(self):
        """(bids [N, K], budget [N]) page-locked arrays: fill them in place and pass them to step() to skip the staging copy"""
        return self._bids_stage, self._budget_stage

    def step_flat(self, flat_actions):
        N, K = self.num_envs, self.num_keywords
        if self._flat_act is None:
            alloc = self.parts[0]._pinned_array
            self._flat_act, self._flat_obs = alloc((N, K + 1), np.float32), alloc((N, 5 * K + 2), np.float32)
        o = self.out
        flat_actions = np.asarray(flat_actions, dtype=np.float32).reshape(N, K + 1)
        for (p, b0, b1), small in zip(self._each(), self._small):
            if not _is_buffer(flat_actions, self._flat_act):
                self._flat_act[b0:b1] = flat_actions[b0:b1]
            p.step_flat_async(self._flat_act[b0:b1].ctypes.data, self._flat_obs[b0:b1].ctypes.data, small["reward"].ctypes.data,
                              small["terminated"].ctypes.data, small["truncated"].ctypes.data)
        self._wait_and_gather()
        return self._flat_obs, o["reward"], o["terminated"], o["truncated"]

    def step_device(self, d_bids=None, d_budget=None):
        if d_bids is not None or d_budget is not None:
            raise NotImplementedError("caller-owned device actions need one engine (engine_shards=1)")
        for p in self.parts:
            p.step_device()


class ReplayTape:
    """Host-side tape for StepEngine.step_replay: the variates the reference drew, in its order."""

    def __init__(self, num_envs, volumes, bid_cents=(), click=(), conv=(), rev_cents=(), x_impressions=(), x_cost=(),
                 offsets=None, drift_uniforms=None):
        N = int(num_envs)
        self.vol = np.ascontiguousarray(volumes, dtype=np.int32)
        self.bid = np.ascontiguousarray(bid_cents, dtype=np.int32)
        self.click = np.ascontiguousarray(click, dtype=np.uint8)
        self.conv = np.ascontiguousarray(conv, dtype=np.uint8)
        self.rev = np.ascontiguousarray(rev_cents, dtype=np.int32)
        self.ximp = np.ascontiguousarray(x_impressions, dtype=np.int32)
        self.xcost = np.ascontiguousarray(x_cost, dtype=np.float64)
        names = ("bid", "ximp", "xcost", "click", "conv", "rev")
        offsets = offsets or {}
        self.off = {n: np.ascontiguousarray(offsets.get(n, np.zeros(N)), dtype=np.int64) for n in names}
        self.end = {n: np.zeros(N, dtype=np.int64) for n in names}
        self.struct = _ffi.Tape(
            self.vol.ctypes.data, self.bid.ctypes.data, self.ximp.ctypes.data, self.xcost.ctypes.data,
            self.click.ctypes.data, self.conv.ctypes.data, self.rev.ctypes.data,
            self.bid.size, self.ximp.size, self.xcost.size, self.click.size, self.conv.size, self.rev.size,
            *(self.off[n].ctypes.data for n in names), *(self.end[n].ctypes.data for n in names), None)
        # the three vectors update_keywords() drew after this step (vol, ctr, cvr; gymnasium_kw_env.py:132-135), [3][N][K]
        self.drift = None if drift_uniforms is None else np.ascontiguousarray(drift_uniforms, dtype=np.float32)
        if self.drift is not None:
            assert self.drift.size == 3 * self.vol.size, "drift_uniforms must be [3][num_envs][num_keywords]"
            self.struct.drift_uniforms = self.drift.ctypes.data


def explicit_curve_host(key, tick, keyword, n_samples, a, b, bid_grid, impression_thresh=0.05):
    """the host twin of an EXPLICIT keyword's cached curve (adc_explicit_curve_host): the draws of the env stream (key, tick)
    that bid_curves_build makes for keyword `keyword`, sorted on the CPU.  Returns (impression_rate, cpc, (z_lo, z_hi))."""
    grid = np.ascontiguousarray(bid_grid, dtype=np.float64)
    ir = np.zeros(grid.size, np.float64)
    cpc = np.zeros(grid.size, np.float64)
    z = np.zeros(2, np.float64)
    check(_ffi.lib().adc_explicit_curve_host(int(key), int(tick), int(keyword), int(n_samples), float(impression_thresh), float(a),
                                             float(b), grid.ctypes.data, grid.size, ir.ctypes.data, cpc.ctypes.data, z.ctypes.data))
    return ir, cpc, (float(z[0]), float(z[1]))
