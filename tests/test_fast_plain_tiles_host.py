"""CPU: what stage B of k_step_implicit_fast leaves out on a PLAIN tile, and the layout of its queue tags.

A keyword-day is plain (adc::fast_keyword_plain, adc_law.h) when it packs (adc::fast_money_packs) and its conversion threshold is
below 2^32.  Wherever the predicate says so, the revenue in cents without money_to_cents's upper clamp (adc::revenue_cents_unclamped)
equals adc::revenue_cents_tab - at the table's extreme words, at random ones and at the law's own bound in dollars - and the single
compare `word < t32` equals the 64-bit test adc::bernoulli(word, T).  No law with T = 2^32 and no law with a NaN is plain.  The tag
of a queued clicked win (adc::fast_tag) gives back its keyword, its accumulator's byte offset and its auction.  Host build of the
kernels' own adc_law.h (g++), as tests/test_fast_packed_money_host.py, whose ranges the laws are drawn over."""
import ctypes as C

import numpy as np
import pytest

from oracle import build as obuild

N_LAWS = 100_000
EXTREME_WORDS = np.array([0x00000000, 0x80000000, 0x000000FF, 0x800000FF, 0xFFFFFFFF, 0x7FFFFFFF, 0x00000100, 0x80000100], np.uint32)
BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
SCTRS = np.array([0.0, 1.0e-12, 0.8, BELOW_ONE, 1.0, np.nan], np.float32)


@pytest.fixture(scope="module")
def L():
    lib = C.CDLL(obuild.build_shims_host())
    vp = C.c_void_p
    lib.adc_fast_plain_tiles_host.argtypes = [C.c_int64, vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_uint64, vp, vp, vp, vp, vp, vp, vp]
    lib.adc_fast_plain_tiles_host.restype = C.c_int
    lib.adc_fast_money_packs_host.argtypes = [C.c_int64, vp, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp]
    lib.adc_fast_money_packs_host.restype = C.c_int
    lib.adc_fast_tag_host.argtypes = [C.c_uint32, C.c_uint32, vp]
    lib.adc_fast_tag_host.restype = C.c_int
    return lib


def _plain(L, V, bid, mu, sd, sctr, words, n_random=1000, seed=7):
    V = np.ascontiguousarray(V, dtype=np.int32)
    bid, mu, sd, sctr = (np.ascontiguousarray(a, dtype=np.float32) for a in (bid, mu, sd, sctr))
    words = np.ascontiguousarray(words, dtype=np.uint32)
    n, nw = V.size, words.size
    out = dict(plain=np.zeros(n, np.uint8), t32=np.zeros(n, np.uint32), T=np.zeros(n, np.uint64), rev_tab=np.full((n, nw), -7, np.int32),
               rev_plain=np.full((n, nw), -9, np.int32), rev_rmax=np.full((n, 2), -7, np.int32), conv_bad=np.full(n, -1, np.int32))
    assert L.adc_fast_plain_tiles_host(n, V.ctypes.data, bid.ctypes.data, mu.ctypes.data, sd.ctypes.data, sctr.ctypes.data, words.ctypes.data, nw,
                                       n_random, seed, *(out[k].ctypes.data for k in ("plain", "t32", "T", "rev_tab", "rev_plain", "rev_rmax", "conv_bad"))) == 0
    packs = np.zeros(n, np.uint8)
    bid_c, r_max = np.zeros(n, np.int32), np.zeros(n, np.int64)
    assert L.adc_fast_money_packs_host(n, V.ctypes.data, bid.ctypes.data, mu.ctypes.data, sd.ctypes.data, None, 0, packs.ctypes.data,
                                       bid_c.ctypes.data, r_max.ctypes.data, None, None) == 0
    out["plain"] = out["plain"].astype(bool)
    out["packs"] = packs.astype(bool)
    return out


def _random_laws(rng, n):
    """the laws of test_fast_packed_money_host.py (mu 1 cent .. $1e6, sd 0 and 1 cent .. $1e5, both signs, bids 1 cent .. 1e9 cents, V
    1 .. 2^20, 1 % NaN / infinite), and a conversion rate: two thirds uniform in (0, 1), the rest from SCTRS"""
    mu = (10.0 ** rng.uniform(-2.0, 6.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    sd = (10.0 ** rng.uniform(-2.0, 5.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    sd[rng.random(n) < 0.1] = 0.0
    bid_cents = np.rint(10.0 ** rng.uniform(0.0, 9.0, n))
    ordinary = rng.random(n) < 0.2
    bid_cents[ordinary] = rng.integers(1, 2001, ordinary.sum())
    bid = (bid_cents / 100.0).astype(np.float32)
    V = np.clip(np.rint(2.0 ** rng.uniform(0.0, 20.0, n)), 1, 2**20).astype(np.int32)
    V[rng.random(n) < 0.02] = 2**20
    odd = np.flatnonzero(rng.random(n) < 0.01)
    special = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), odd.size)
    in_mu = rng.random(odd.size) < 0.5
    mu[odd[in_mu]] = special[in_mu]
    sd[odd[~in_mu]] = special[~in_mu]
    sctr = rng.uniform(0.0, 1.0, n).astype(np.float32)
    pick = rng.random(n) < 1.0 / 3.0
    sctr[pick] = rng.choice(SCTRS, int(pick.sum()))
    return V, bid, mu, sd, sctr


def test_plain_laws_need_neither_guard(L):
    rng = np.random.default_rng(5151)
    V, bid, mu, sd, sctr = _random_laws(rng, N_LAWS)
    words = np.concatenate([EXTREME_WORDS, rng.integers(0, 2**32, 8, dtype=np.uint64).astype(np.uint32)])
    o = _plain(L, V, bid, mu, sd, sctr, words)
    p = o["plain"]
    print(f"plain: {p.mean():.4f} of {p.size} laws; not plain: {(~p).mean():.4f} (packing: {o['packs'].mean():.4f})")
    assert p.sum() >= N_LAWS // 3 and (~p).sum() >= N_LAWS // 10
    # the thresholds, from the rate alone (float64: p 2^32 is exact)
    with np.errstate(invalid="ignore"):
        T_ref = np.where(sctr > 0, np.minimum(np.floor(sctr.astype(np.float64) * 2.0**32 + 0.5), 2.0**32), 0.0)
    T_ref = np.where(np.isnan(sctr), 0.0, T_ref).astype(np.uint64)
    assert (o["T"] == T_ref).all()
    assert (o["t32"] == np.minimum(T_ref, 2**32 - 1).astype(np.uint32)).all()
    for s, want in ((0.0, 0), (0.8, 13421773 * 256), (BELOW_ONE, 2**32 - 256), (1.0, 2**32)):
        assert (o["T"][sctr == np.float32(s)] == want).all() and (sctr == np.float32(s)).sum() > 1000
    # the predicate is what it says: packing, a threshold below 2^32, no NaN
    always = o["T"] == 2**32
    nan = np.isnan(mu) | np.isnan(sd) | np.isnan(sctr)
    assert always.sum() > 1000 and nan.sum() > 1000
    assert not p[always].any() and not p[nan].any() and not p[~o["packs"]].any()
    assert (p == (o["packs"] & ~always & ~nan)).all()
    # wherever it says plain: the unclamped revenue is the shared routine's, at every word and at the law's own bound
    assert (o["rev_plain"][p] == o["rev_tab"][p]).all() and (o["rev_tab"][p] >= 1).all()
    assert (o["rev_rmax"][p, 0] == o["rev_rmax"][p, 1]).all() and (o["rev_rmax"][p, 0] >= 0).all()
    assert o["rev_rmax"][p, 0].max() > 10**7          # (bounds above $100 000 are among them)
    # and one compare is the 64-bit test, at 0, T - 1, T, 2^32 - 2, 2^32 - 1 and 1000 random words
    assert (o["conv_bad"][p] == 0).all()
    # the check can fail: with T = 2^32 the word 2^32 - 1 (given twice: it is T - 1 too) converts, and is not below 0xFFFFFFFF
    assert (o["conv_bad"][always] == 2).all()
    assert (o["conv_bad"][~always] == 0).all()


def test_plain_edges(L):
    """the largest revenue bound that packs at all (just under 1e7 dollars, one auction), a bound of 1e7, and each special rate"""
    nine = float(np.nextafter(np.float32(1.0e7), np.float32(0.0)))
    V = np.array([1, 1, 1, 40, 40, 40, 40, 40, 40], np.int32)
    bid = np.array([0.5] * 9, np.float32)
    mu = np.array([nine, 1.0e7, 9.9e6, 30.0, 30.0, 30.0, 30.0, 30.0, np.nan], np.float32)
    sd = np.array([0.0, 0.0, 1.0e3, 10.0, 10.0, 10.0, 10.0, 10.0, 10.0], np.float32)
    sctr = np.array([0.5, 0.5, 0.5, 0.0, 1.0e-12, BELOW_ONE, 1.0, np.nan, 0.5], np.float32)
    o = _plain(L, V, bid, mu, sd, sctr, EXTREME_WORDS)
    assert o["plain"].tolist() == [True, False, True, True, True, True, False, False, False]
    assert o["rev_rmax"][0].tolist() == [999999872, 999999872]          # 9 999 999 dollars x 100, rounded to float32: below the clamp's 1e9
    assert (o["rev_plain"][0] == 999999872).all() and (o["rev_tab"][0] == 999999872).all()
    assert (o["rev_plain"][2] == o["rev_tab"][2]).all() and o["rev_tab"][2].max() > 990_000_000
    assert o["T"].tolist()[3:8] == [0, 0, 2**32 - 256, 2**32, 0]
    assert (o["conv_bad"][o["plain"]] == 0).all()


def test_tag_layout_round_trips(L):
    out = np.zeros(4, np.uint32)
    seen = set()
    for j in (0, 1, 2**20 - 1, 2**20):
        for u in range(256):
            assert L.adc_fast_tag_host(u, j, out.ctypes.data) == 0
            tag, acc_off, kw, auction = (int(x) for x in out)
            assert tag == (j << 11 | u << 3) and tag < 2**32
            assert (acc_off, kw, auction) == (8 * u, u, j)
            seen.add(tag)
    assert len(seen) == 4 * 256
    assert L.adc_fast_tag_host(256, 0, out.ctypes.data) != 0 and L.adc_fast_tag_host(0, 2**20 + 1, out.ctypes.data) != 0
