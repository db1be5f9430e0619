"""adc_law.h lower_bound_v (a window from one table evaluation, three accepting evaluations, a neighbourhood, then the
bisection) against lower_bound_v_bisect (the verified-window bisection alone, the routine every earlier result was computed
with): the same value on every input, and the same win intervals field by field.  Host code only (oracle/build.py
build_shims_host: adc_shims.cpp + adc_law.h by g++); the copy hipcc builds into the library is compared on a sample where the
library is present (tests/test_shims_host_build.py does the same for the older shims).

Shares measured here on the cfg2 laws (synthetic.implicit_keyword_planes, bids round2(U(0.3, 1.0)), 10^7 bounds / 10^6 keywords,
also in profiles/pr_fast_law_setup.txt): a keyword leaves the accepting stage with p = 2.3e-6, a wave of 64 with
1 - (1 - p)^64 = 1.5e-4; no keyword reaches the bisection."""
import ctypes as C

import numpy as np
import pytest

from adcraft_amd import gymnasium_kw_utils as kwu
from adcraft_amd import synthetic
from oracle import build as obuild

TOP = 1 << 24


@pytest.fixture(scope="module")
def H():
    L = C.CDLL(obuild.build_shims_host())
    i64, i32, vp = C.c_int64, C.c_int32, C.c_void_p
    for name, args in {"adc_lower_bound_v_host": [i64, vp, vp, vp, vp, vp], "adc_lower_bound_v_bisect_host": [i64, vp, vp, vp, vp, vp],
                       "adc_win_intervals_host": [i64, vp, vp, vp, vp, i32, vp, vp]}.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = args, C.c_int
    return L


def _both(L, target, loc, scale):
    """(new value, stage, old value, old routine fell back to its whole-range bisection) for arrays of equal length"""
    target = np.ascontiguousarray(target, np.int32)
    loc = np.ascontiguousarray(loc, np.float32)
    scale = np.ascontiguousarray(scale, np.float32)
    n = target.size
    assert loc.size == n and scale.size == n
    new, old = np.empty(n, np.uint32), np.empty(n, np.uint32)
    stage, whole = np.empty(n, np.uint8), np.empty(n, np.uint8)
    p = lambda a: a.ctypes.data
    assert L.adc_lower_bound_v_host(n, p(target), p(loc), p(scale), p(new), p(stage)) == 0
    assert L.adc_lower_bound_v_bisect_host(n, p(target), p(loc), p(scale), p(old), p(whole)) == 0
    return new, stage, old, whole


def _assert_same(new, old, target, loc, scale):
    bad = np.flatnonzero(new != old)
    assert bad.size == 0, (bad.size, [(int(target[i]), float(loc[i]), float(scale[i]), int(new[i]), int(old[i])) for i in bad[:5]])
    assert int(new.max()) <= TOP


def _cfg2_laws(rng, n):
    """loc, scale of synthetic.implicit_keyword_planes (the benchmark's keyword law) and the bids bench.py steps with"""
    planes = synthetic.implicit_keyword_planes(n // 256, 256, seed=int(rng.integers(1 << 30)))
    loc, scale = planes[2].ravel(), planes[3].ravel()
    bid_c = np.rint(rng.uniform(0.3, 1.0, loc.size).astype(np.float32) * 100.0).astype(np.int32)
    return bid_c, loc, scale


def _quantile_laws(rng, n):
    """the same quantile law as gymnasium_kw_utils draws it (sample_implicit_keyword_params on the experiment table), vectorised,
    with the wider bids an agent may place (1 cent to 3 dollars)"""
    t = kwu.generate_simple_experiment_quantiles(128, 0.8)
    q = lambda name: np.interp(rng.random(n), [0.0, 0.5, 1.0], [t[f"min_{name}"][0], t[f"median_{name}"][0], t[f"max_{name}"][0]])
    loc = q("ave_cpc")
    scale = np.maximum(0.01, q("std_cpc") * loc)
    return rng.integers(1, 301, n).astype(np.int32), loc.astype(np.float32), scale.astype(np.float32)


def test_random_laws_ten_million(H):
    """>= 10^7 (target, loc, scale): both targets (1 - bid, bid) of keywords of the cfg2 law and of the quantile law as
    gymnasium_kw_utils samples it, a sample drawn by sample_implicit_keyword_params itself, and log-uniform wide ranges"""
    rng = np.random.default_rng(2024)
    total = 0
    for laws, n in ((_cfg2_laws, 2_560_000), (_quantile_laws, 2_000_000)):
        bid_c, loc, scale = laws(rng, n)
        for target in (1 - bid_c, bid_c):
            new, stage, old, whole = _both(H, target, loc, scale)
            _assert_same(new, old, target, loc, scale)
            assert not whole.any()
            total += target.size
    params = kwu.sample_implicit_keyword_params(2000, np.random.default_rng(5), kwu.experiment_keyword_config(128, 0.8))
    loc = np.array([p[1] for p in params], np.float32)
    scale = np.array([p[2] for p in params], np.float32)
    bid_c = rng.integers(1, 200, loc.size).astype(np.int32)
    for target in (1 - bid_c, bid_c):
        new, stage, old, whole = _both(H, target, loc, scale)
        _assert_same(new, old, target, loc, scale)
        total += target.size
    n = 1_000_000
    target = np.where(rng.random(n) < 0.5, 1, -1) * np.rint(np.exp(rng.uniform(0, np.log(1e9), n))).astype(np.int64)
    loc = np.exp(rng.uniform(-6, 6, n)) * rng.choice([-1.0, 1.0], n, p=[0.2, 0.8])
    scale = np.exp(rng.uniform(-14, 5, n)) * rng.choice([-1.0, 1.0], n, p=[0.1, 0.9])
    new, stage, old, whole = _both(H, target, loc, scale)
    _assert_same(new, old, target, loc, scale)
    total += n
    assert total >= 10_000_000


def test_adversarial_inputs(H):
    """|scale| at 0, denormal, 1e-6 and huge; NaN and +-inf in loc or scale; targets 1 - bid and bid for bids of 0, 1 and 10^9
    cents (and their neighbours); every combination"""
    scales = [0.0, -0.0, 1e-45, 1e-40, 1.1754944e-38, 1e-6, -1e-6, 0.01, 0.08, -0.08, 1.0, 50.0, 1e6, 1e30, 3.4e38, np.inf, -np.inf, np.nan]
    locs = [0.0, -0.0, 1e-45, 0.005, -0.005, 0.3, 0.55, 0.64, 1.0, -0.4, 3.0, 1e4, -1e4, 1e7, 1.0e7 + 1, 1e30, np.inf, -np.inf, np.nan]
    targets = []
    for bid in (0, 1, 2, 64, 70, 10**9 - 1, 10**9):
        targets += [1 - bid, bid]
    targets += [-(2**31), -(2**31) + 1, 2**31 - 1, 10**9 + 1, -(10**9) - 1, 2**24, 2**24 + 1, -(2**24) - 1]
    T, Lc, S = np.meshgrid(np.array(targets, np.int64), np.array(locs, np.float32), np.array(scales, np.float32), indexing="ij")
    new, stage, old, whole = _both(H, T.ravel(), Lc.ravel(), S.ravel())
    _assert_same(new, old, T.ravel(), Lc.ravel(), S.ravel())
    assert {0, TOP} <= set(int(x) for x in np.unique(new))


def test_answers_at_the_ends_and_the_middle_of_the_range(H):
    """targets chosen so that the bound itself is 0, 1, 2^23 - 1, 2^23, 2^23 + 1, 2^24 - 1 and 2^24: the target is set to the signed
    cents the law gives at that v (read off the old routine's own monotone search: W(S(v)) <= v < W(S(v) + 1)), so the answer
    sits at or next to the wanted v; every wanted value must occur"""
    rng = np.random.default_rng(77)
    n = 40_000
    seen = set()
    for want in (0, 1, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, TOP - 1, TOP):
        loc = rng.uniform(0.3, 1.0, n).astype(np.float32)
        scale = (loc * rng.uniform(0.01, 0.3, n)).astype(np.float32)
        if 1 < want < TOP - 1:          # around 2^23 the deviate moves by 1.2e-7 per v: only a huge scale tells neighbours apart
            scale = np.exp(rng.uniform(np.log(1e6), np.log(1e9), n)).astype(np.float32)
        # bisect on the target: the largest target whose bound is <= want - then the bound of target + 1 is > want, and one
        # of the two is often want itself
        lo, hi = np.full(n, -(10**9), np.int64), np.full(n, 10**9, np.int64)
        for _ in range(32):
            mid = (lo + hi + 1) >> 1
            _, _, old, _ = _both(H, mid, loc, scale)
            ok = old <= want
            lo = np.where(ok, mid, lo)
            hi = np.where(ok, hi, mid - 1)
        for target in (lo - 1, lo, lo + 1):
            target = np.clip(target, -(2**31), 2**31 - 1)
            new, stage, old, whole = _both(H, target, loc, scale)
            _assert_same(new, old, target, loc, scale)
            seen |= set(int(x) for x in np.unique(new))
    assert {0, 1, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, TOP - 1, TOP} <= seen


def _intervals(L, bid_c, loc, scale, ctr, bisect):
    n = bid_c.size
    out, stage = np.empty((n, 4), np.uint32), np.empty(n, np.uint8)
    p = lambda a: a.ctypes.data
    assert L.adc_win_intervals_host(n, p(bid_c), p(loc), p(scale), p(ctr), bisect, p(out), p(stage)) == 0
    return out, stage


def test_win_intervals_field_by_field_and_the_share_off_the_common_path(H):
    """win_intervals on 1.28 10^6 keywords of the cfg2 law (and 3 10^5 of wide / degenerate ones), old against new, field by
    field.  On the cfg2 keywords: p = the share of keywords whose bounds are not both settled by the accepting evaluations, and
    the share of waves of 64 keywords that then enter the rare stages, 1 - (1 - p)^64: below one wave in ten (none of these
    keywords sends the old routine to its whole-range bisection)."""
    rng = np.random.default_rng(404)
    bid_c, loc, scale = _cfg2_laws(rng, 1_280_000)
    n = bid_c.size
    assert n >= 1_000_000
    ctr = np.interp(rng.random(n), [0.0, 0.5, 1.0], [0.1, 0.5, 0.9]).astype(np.float32)
    new, stage = _intervals(H, bid_c, loc, scale, ctr, 0)
    old, whole = _intervals(H, bid_c, loc, scale, ctr, 1)
    for f, name in enumerate(("c_lo", "c_w", "n_lo", "n_w")):
        assert np.array_equal(new[:, f], old[:, f]), name
    assert not whole.any()
    p = float(np.mean(stage != 0))
    p_bisect = float(np.mean(stage == 2))
    wave = 1.0 - (1.0 - p) ** 64
    waves_seen = float(np.mean(stage.reshape(-1, 64).max(axis=1) != 0))          # the keywords as the kernel's waves hold them
    print(f"cfg2 law, {n} keywords: off the accepting stage p = {p:.3g} (bisection {p_bisect:.3g}); per wave 1 - (1 - p)^64 = {wave:.3g}, "
          f"counted over consecutive 64s {waves_seen:.3g}")
    assert wave < 0.1 and waves_seen < 0.1
    # wide and degenerate keywords: equality only
    m = 300_000
    bid2 = np.rint(np.exp(rng.uniform(0, np.log(1e9), m))).astype(np.int32)
    loc2 = (np.exp(rng.uniform(-5, 5, m)) * rng.choice([-1.0, 1.0], m, p=[0.2, 0.8])).astype(np.float32)
    scale2 = np.exp(rng.uniform(-14, 4, m)).astype(np.float32)
    ctr2 = np.where(rng.random(m) < 0.2, rng.choice([0.0, 1.0, 1e-9, 1.0 - 1e-7], m), rng.random(m)).astype(np.float32)
    for arr, vals in ((loc2, [np.nan, np.inf, -np.inf, 0.0]), (scale2, [np.nan, np.inf, 0.0, -0.08, 1e-40])):
        idx = rng.integers(0, m, 8 * len(vals))
        arr[idx] = np.tile(np.array(vals, np.float32), 8)
    new, _ = _intervals(H, bid2, loc2, scale2, ctr2, 0)
    old, _ = _intervals(H, bid2, loc2, scale2, ctr2, 1)
    assert np.array_equal(new, old)


def test_the_librarys_copy_gives_the_same_bits(H):
    """the copy of these shims that hipcc builds into the library (clang, its own exp2f and division) against the g++ build:
    equal values - the estimate's last bits reach no result"""
    from adcraft_amd import _ffi
    P = _ffi.lib()
    rng = np.random.default_rng(9)
    bid_c, loc, scale = _quantile_laws(rng, 50_000)
    loc[:8] = [np.nan, np.inf, 0.0, 1e7, -1.0, 0.5, 0.5, 0.5]
    scale[:8] = [0.1, 0.1, 0.0, 1e-6, 50.0, np.nan, np.inf, 1e-40]
    n = bid_c.size
    p = lambda a: a.ctypes.data
    for target in (1 - bid_c, bid_c):
        target = np.ascontiguousarray(target, np.int32)
        new, stage, old, whole = _both(H, target, loc, scale)
        v, st = np.empty(n, np.uint32), np.empty(n, np.uint8)
        assert P.adc_lower_bound_v_host(n, p(target), p(loc), p(scale), p(v), p(st)) == 0
        assert np.array_equal(v, new) and np.array_equal(v, old)
        assert P.adc_lower_bound_v_bisect_host(n, p(target), p(loc), p(scale), p(v), None) == 0
        assert np.array_equal(v, old)
