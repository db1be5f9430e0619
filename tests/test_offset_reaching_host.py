"""adc_law.h offset_reaching (a float32 candidate for ceil(W 2^32 / m), accepted on its exact 64-bit residual; the float64
routine behind a ballot) against offset_reaching_f64 (the float64 division every earlier result was computed with): the same
value on every input, and the same win intervals field by field on the benchmark's keywords.  Host code only (oracle/build.py
build_shims_host: adc_shims.cpp + adc_law.h by g++); the copy hipcc builds into the library is compared on a sample.

The share of the float64 path is a condition here, not a measurement: on the cfg2 keywords fewer than 1 % of the groups of 64
consecutive keywords (the kernel's waves) may hold a keyword that takes it.  Measured: none (profiles/pr_fast_offsets.txt)."""
import ctypes as C

import numpy as np
import pytest

from adcraft_amd import synthetic
from oracle import build as obuild

TOP = 1 << 24
TWO32 = 1 << 32
M_SAT = 4294967040


@pytest.fixture(scope="module")
def H():
    L = C.CDLL(obuild.build_shims_host())
    i64, i32, vp = C.c_int64, C.c_int32, C.c_void_p
    for name, args in {"adc_offset_reaching_host": [i64, vp, vp, vp, vp, vp], "adc_offset_reaching_f64_host": [i64, vp, vp, vp, vp, vp],
                       "adc_win_intervals_offsets_host": [i64, vp, vp, vp, vp, i32, vp, vp]}.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = args, C.c_int
    return L


def _multiplier(rng_):
    """adc::rescale_multiplier: floor(2^56 / range) in float32 (one correctly rounded division), saturated; 0 for range 0"""
    rng_ = np.asarray(rng_, np.uint64)
    with np.errstate(divide="ignore"):
        m = np.floor(np.float32(2.0**56) / rng_.astype(np.float32))
    m = np.minimum(m, np.float32(M_SAT)).astype(np.float64)
    return np.where(rng_ == 0, 0, m).astype(np.uint32)


def _both(L, W, m, rng_):
    """(new value, new path, float64 value, float64 path) for arrays of equal length"""
    W = np.ascontiguousarray(W, np.uint32)
    m = np.ascontiguousarray(m, np.uint32)
    rng_ = np.ascontiguousarray(rng_, np.uint64)
    n = W.size
    assert m.size == n and rng_.size == n
    new, old = np.empty(n, np.uint64), np.empty(n, np.uint64)
    path, path64 = np.empty(n, np.uint8), np.empty(n, np.uint8)
    p = lambda a: a.ctypes.data
    assert L.adc_offset_reaching_host(n, p(W), p(m), p(rng_), p(new), p(path)) == 0
    assert L.adc_offset_reaching_f64_host(n, p(W), p(m), p(rng_), p(old), p(path64)) == 0
    return new, path, old, path64


def _assert_same(new, old, W, m, rng_):
    bad = np.flatnonzero(new != old)
    assert bad.size == 0, (bad.size, [(int(W[i]), int(m[i]), int(rng_[i]), int(new[i]), int(old[i])) for i in bad[:5]])
    assert np.all(new <= np.asarray(rng_, np.uint64))


def _exact(W, m, rng_):
    """the definition in Python integers"""
    if W == 0:
        return 0
    if W > TOP - 1 or m == 0:
        return rng_
    return min(-((-W << 32) // m), rng_)


def _thresholds(rng, n):
    """T = round(ctr 2^32) for click rates as the laws have them: the benchmark's (0.1 .. 0.9), uniform, and log-uniform small
    ones on either side (ranges below 2^24 saturate the multiplier)"""
    kind = rng.integers(0, 4, n)
    ctr = np.where(kind == 0, np.interp(rng.random(n), [0.0, 0.5, 1.0], [0.1, 0.5, 0.9]), rng.random(n))
    small = np.exp(rng.uniform(np.log(2.0**-32), 0.0, n))
    ctr = np.where(kind == 2, small, np.where(kind == 3, 1.0 - small, ctr)).astype(np.float32)
    return np.clip(np.rint(ctr.astype(np.float64) * 2.0**32), 0, 2.0**32).astype(np.uint64)


def test_random_triples_ten_million(H):
    """>= 10^7 (W, m, range) as the kernels make them: range = T and 2^32 - T, m = rescale_multiplier(range), W uniform on
    [0, 2^24] with the ends over-weighted.  Candidate-path values are also checked against the integer definition on a sample."""
    rng = np.random.default_rng(2025)
    total = 0
    f64_share = []
    for _ in range(5):
        n = 1_100_000
        T = _thresholds(rng, n)
        W = rng.integers(0, TOP + 1, n).astype(np.uint32)
        ends = rng.random(n) < 0.02
        W[ends] = rng.choice(np.array([0, 1, 2, TOP - 2, TOP - 1, TOP], np.uint32), int(ends.sum()))
        for rng_ in (T, np.uint64(TWO32) - T):
            m = _multiplier(rng_)
            new, path, old, _ = _both(H, W, m, rng_)
            _assert_same(new, old, W, m, rng_)
            f64_share.append(float(np.mean(path != 0)))
            assert np.array_equal(path != 0, (m == 0) & (W < TOP))          # a law's multiplier is 0 (click rate 0 or 1) or >= 2^24
            for i in rng.integers(0, n, 2000):
                assert int(new[i]) == _exact(int(W[i]), int(m[i]), int(rng_[i]))
            total += n
    assert total >= 10_000_000
    print(f"float64 path on {total} random triples: {np.mean(f64_share):.3g}")


def test_adversarial_grid(H):
    """every W of the end set with every T of the end set (both ranges), with the saturated multiplier, and with m == 0 and
    multipliers no law produces (below 2^24, where the quotient leaves 32 bits: the float64 routine's share)"""
    Ws = [0, 1, 2, TOP - 1, TOP, TOP + 1, 2**31, 2**32 - 1]
    Ts = [0, 1, TOP - 1, TOP, TOP + 1, 2**31, TWO32 - 256, TWO32]
    ranges = sorted(set(Ts) | {TWO32 - t for t in Ts} | {255, 256, 257, 2**31 - 1, 2**31 + 1, TWO32 - 1})
    ms = sorted({int(x) for x in _multiplier(np.array(ranges, np.uint64))} | {0, 1, 2, 3, 255, 2**16, TOP - 1, TOP, TOP + 1, 2**31, M_SAT, M_SAT + 1, 2**32 - 1})
    Wg, Mg, Rg = np.meshgrid(np.array(Ws, np.uint32), np.array(ms, np.uint32), np.array(ranges, np.uint64), indexing="ij")
    W, m, rng_ = Wg.ravel(), Mg.ravel(), Rg.ravel()
    new, path, old, path64 = _both(H, W, m, rng_)
    _assert_same(new, old, W, m, rng_)
    for i in range(W.size):
        assert int(new[i]) == _exact(int(W[i]), int(m[i]), int(rng_[i]))
    assert set(np.unique(path)) == {0, 1} and set(np.unique(path64)) == {0, 1, 2, 3}
    # the float64 routine's share: the multipliers below 2^24 (of a law's, only 0), unless W is beyond every offset
    assert np.array_equal(path != 0, (m < TOP) & (W < TOP))


def test_every_w_next_to_an_exact_multiple(H):
    """for each multiplier of the end-set thresholds, the saturated one and some of the benchmark's: every W in [1, 2^24) whose
    quotient W 2^32 / m lies within 2^-9 of an integer (the residue within m / 512 of a multiple of m: far more than the
    float32 correction's error, and a superset of the residues within 2), plus that W's neighbours - where the candidate has
    to move by one.  Both an ample range and one that cuts the quotient off."""
    rng = np.random.default_rng(31)
    Ts = np.array([1, TOP - 1, TOP, TOP + 1, 2**31, TWO32 - 256, TWO32], np.uint64)
    ranges = np.concatenate([Ts, np.uint64(TWO32) - Ts[:-1], _thresholds(rng, 16)])
    ms = sorted({int(x) for x in _multiplier(ranges)} | {M_SAT})
    assert M_SAT in ms and TOP in ms and 0 not in ms
    allW = np.arange(1, TOP, dtype=np.uint64)
    moved = 0
    for m_ in ms:
        res = (allW << np.uint64(32)) % np.uint64(m_)
        near = np.flatnonzero((res <= np.uint64(max(2, m_ >> 9))) | (res >= np.uint64(m_ - max(2, m_ >> 9))))
        W = np.unique(np.clip(np.concatenate([allW[near] - 1, allW[near], allW[near] + 1]), 1, TOP - 1)).astype(np.uint32)
        m = np.full(W.size, m_, np.uint32)
        for rng_ in (np.full(W.size, TWO32, np.uint64), np.full(W.size, (int(W[W.size // 2]) << 32) // m_, np.uint64)):
            new, path, old, _ = _both(H, W, m, rng_)
            _assert_same(new, old, W, m, rng_)
            assert not path.any()
        # (new and rng_ of the cut-off range) where the division is exact the quotient itself is the answer
        q = (W.astype(np.uint64) << np.uint64(32)) // np.uint64(m_)
        exact = np.flatnonzero((W.astype(np.uint64) << np.uint64(32)) % np.uint64(m_) == 0)
        assert np.array_equal(new[exact], np.minimum(q[exact], rng_[exact]))
        moved += W.size
    assert moved > 100_000 and len(ms) >= 16


def _cfg2_keywords():
    """the planes bench.py builds for cfg2 and bids of its sample_actions(0.30, 1.00) law: round2(U(0.3, 1.0)) in cents"""
    planes = synthetic.implicit_keyword_planes(4096, 256, seed=1729)
    loc, scale, ctr = planes[2].ravel(), planes[3].ravel(), planes[4].ravel()
    bid_c = np.rint(np.random.default_rng(1729).uniform(0.30, 1.00, loc.size).astype(np.float32) * 100.0).astype(np.int32)
    return bid_c, np.ascontiguousarray(loc), np.ascontiguousarray(scale), np.ascontiguousarray(ctr)


def _intervals(L, bid_c, loc, scale, ctr, f64):
    n = bid_c.size
    out, path = np.empty((n, 4), np.uint32), np.empty(n, np.uint8)
    p = lambda a: a.ctypes.data
    assert L.adc_win_intervals_offsets_host(n, p(bid_c), p(loc), p(scale), p(ctr), f64, p(out), p(path)) == 0
    return out, path


def test_win_intervals_of_cfg2_and_the_float64_share(H):
    """win_intervals on the 2^20 keywords of cfg2 (seed 1729): the four fields against the float64 form's, and the share of
    64-keyword groups with a keyword on the float64 path below 1 %.  Then wide and degenerate keywords: equality only."""
    bid_c, loc, scale, ctr = _cfg2_keywords()
    new, path = _intervals(H, bid_c, loc, scale, ctr, 0)
    old, path64 = _intervals(H, bid_c, loc, scale, ctr, 1)
    for f, name in enumerate(("c_lo", "c_w", "n_lo", "n_w")):
        assert np.array_equal(new[:, f], old[:, f]), name
    assert path64.all()
    assert (new[:, 1] > 0).mean() > 0.5          # (the keywords do win auctions: the offsets were computed)
    groups = float(np.mean(path.reshape(-1, 64).max(axis=1) != 0))
    print(f"cfg2, {bid_c.size} keywords: float64 path in {float(np.mean(path != 0)):.3g} of keywords, {groups:.3g} of 64-keyword groups")
    assert groups < 0.01
    rng = np.random.default_rng(405)
    m = 300_000
    bid2 = np.rint(np.exp(rng.uniform(0, np.log(1e9), m))).astype(np.int32)
    loc2 = (np.exp(rng.uniform(-5, 5, m)) * rng.choice([-1.0, 1.0], m, p=[0.2, 0.8])).astype(np.float32)
    scale2 = np.exp(rng.uniform(-14, 4, m)).astype(np.float32)
    ctr2 = np.where(rng.random(m) < 0.3, rng.choice([0.0, 1.0, 1e-9, 2.0**-30, 1.0 - 2.0**-24, 1.0 - 1e-7], m), rng.random(m)).astype(np.float32)
    new, _ = _intervals(H, bid2, loc2, scale2, ctr2, 0)
    old, _ = _intervals(H, bid2, loc2, scale2, ctr2, 1)
    assert np.array_equal(new, old)


def test_the_librarys_copy_gives_the_same_bits(H):
    """the copy of the shims that hipcc builds into the library (clang's host code) against the g++ build: equal values and paths"""
    from adcraft_amd import _ffi
    P = _ffi.lib()
    for name in ("adc_offset_reaching_host", "adc_offset_reaching_f64_host"):          # (test exports: not in _ffi's table, so that an
        fn = getattr(P, name)                                                           # earlier build still loads for A/B timing)
        fn.argtypes, fn.restype = [C.c_int64] + [C.c_void_p] * 5, C.c_int
    rng = np.random.default_rng(10)
    n = 200_000
    T = _thresholds(rng, n)
    W = rng.integers(0, TOP + 1, n).astype(np.uint32)
    m = _multiplier(T)
    m[:6] = [0, 1, 255, TOP - 1, M_SAT, 2**32 - 1]
    new, path, old, path64 = _both(H, W, m, T)
    d, pth = np.empty(n, np.uint64), np.empty(n, np.uint8)
    p = lambda a: a.ctypes.data
    assert P.adc_offset_reaching_host(n, p(W), p(m), p(T), p(d), p(pth)) == 0
    assert np.array_equal(d, new) and np.array_equal(pth, path)
    assert P.adc_offset_reaching_f64_host(n, p(W), p(m), p(T), p(d), p(pth)) == 0
    assert np.array_equal(d, old) and np.array_equal(pth, path64)
