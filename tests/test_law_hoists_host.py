"""CPU: what the dense fast pass (k_step_implicit_fast) hoists out of its per-auction stages, through the g++ build of the shims
(adc_shims.cpp calls the routines of csrc/adc_law.h that the kernel calls):
  * adc::draw_folded / adc::draw_kw_folded - a Philox call from the folded word tick ^ key_hi - give the bits of adc::draw;
  * adc::competitor_cents_of_proven_win - the price without its clamp - equals adc::competitor_cents_from_v at every value of a
    keyword's win range, which is where the kernel uses it."""
import ctypes as C

import numpy as np
import pytest

from oracle import build as obuild

N_RANDOM = 1 << 20          # (>= 1e6 cases per property)
STAGES = np.arange(16, dtype=np.uint32)     # every stage of the stream (the IMPLICIT model's five - ST_VOL, ST_AUCTION, ST_DRIFT, ST_METRIC, ST_CONV - among them)


@pytest.fixture(scope="module")
def L():
    lib = C.CDLL(obuild.build_shims_host())
    vp = C.c_void_p
    lib.adc_draw_folded_host.argtypes = [C.c_int64] + [vp] * 8
    lib.adc_draw_folded_host.restype = C.c_int
    lib.adc_proven_win_price_host.argtypes = [C.c_int64, vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, C.c_uint64, vp, vp]
    lib.adc_proven_win_price_host.restype = C.c_int64
    return lib


def p(a):
    return a.ctypes.data


# ---- the folded-word draw ------------------------------------------------------------------------------------------------------
def draws(L, key, index, stage, keyword, tick):
    key, index, stage, keyword, tick = (np.ascontiguousarray(a, dtype=t) for a, t in
                                        ((key, np.uint64), (index, np.uint32), (stage, np.uint32), (keyword, np.uint32), (tick, np.uint32)))
    n = key.size
    assert index.size == n and stage.size == n and keyword.size == n and tick.size == n
    out = [np.zeros((n, 4), np.uint32) for _ in range(3)]
    assert L.adc_draw_folded_host(n, p(key), p(index), p(stage), p(keyword), p(tick), p(out[0]), p(out[1]), p(out[2])) == 0
    return out


def test_folded_draws_give_the_bits_of_draw_on_random_calls(L):
    rng = np.random.default_rng(20240607)
    n = N_RANDOM
    key = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    key[: n // 4] |= np.uint64(0xFFFF0000FFFF0000)                     # high bits of both key halves set
    index = rng.integers(0, (1 << 18) + 1, n, dtype=np.uint32)         # auction / call indices up to 2^18
    keyword = rng.integers(0, 4096, n, dtype=np.uint32)
    stage = STAGES[rng.integers(0, STAGES.size, n)]
    tick = rng.integers(0, 1 << 32, n, dtype=np.uint32)
    plain, folded, kw = draws(L, key, index, stage, keyword, tick)
    assert len(np.unique(plain[:, 0])) > n // 2                         # (the shim did draw)
    assert np.array_equal(folded, plain)
    assert np.array_equal(kw, plain)


def test_folded_draws_at_the_edges_of_every_argument(L):
    keys = np.array([0, 1, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF00000000, 0x00000000FFFFFFFF, 0x8000000080000000, 0x9E3779B97F4A7C15], np.uint64)
    ticks = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)
    indices = np.array([0, 1, 3, 4, (1 << 18) - 1, 1 << 18, 0x00FFFFFF, 0xFFFFFFFF], np.uint32)
    keywords = np.array([0, 1, 255, 256, 4095, 0xFFFFFFFF], np.uint32)
    g = np.meshgrid(keys, indices, STAGES, keywords, ticks, indexing="ij")
    plain, folded, kw = draws(L, *(a.ravel() for a in g))
    assert plain.shape[0] == keys.size * ticks.size * indices.size * keywords.size * STAGES.size
    assert np.array_equal(folded, plain)
    assert np.array_equal(kw, plain)


def test_the_folded_word_is_all_the_draw_reads_of_tick_and_key_hi(L):
    """two (key_hi, tick) pairs with the same xor differ in the later rounds' keys: the fold must not be mistaken for the key"""
    key = np.array([0x0000000100000005, 0x0000000300000005], np.uint64)
    tick = np.array([2, 0], np.uint32)                                  # 1 ^ 2 == 3 ^ 0
    z = np.zeros(2, np.uint32)
    plain, folded, kw = draws(L, key, z, z + 7, z, tick)
    assert not np.array_equal(plain[0], plain[1])
    assert np.array_equal(folded, plain) and np.array_equal(kw, plain)


# ---- the unclamped price of a proven win -----------------------------------------------------------------------------------------
def proven(L, bid_c, loc, scale, bctr, exhaustive_below, ends, samples, seed=1):
    bid_c = np.ascontiguousarray(bid_c, np.int32)
    loc, scale, bctr = (np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32), bid_c.shape)) for a in (loc, scale, bctr))
    checked, first = np.zeros(1, np.int64), np.zeros(3, np.int64)
    bad = L.adc_proven_win_price_host(bid_c.size, p(bid_c), p(loc), p(scale), p(bctr), exhaustive_below, ends, samples, seed, p(checked), p(first))
    assert bad >= 0
    return bad, int(checked[0]), first


def test_unclamped_price_on_random_keywords(L):
    rng = np.random.default_rng(7)
    n = N_RANDOM // 4
    bid_c = np.concatenate([rng.integers(1, 2000, n // 2), np.exp(rng.uniform(0.0, np.log(1.0e9), n - n // 2)).astype(np.int64)]).astype(np.int32)
    loc = rng.uniform(-3.0, 12.0, n).astype(np.float32)
    scale = np.exp(rng.uniform(np.log(1e-3), np.log(50.0), n)).astype(np.float32)
    bctr = rng.uniform(0.0, 1.0, n).astype(np.float32)
    bad, checked, first = proven(L, bid_c, loc, scale, bctr, exhaustive_below=64, ends=4, samples=4)
    assert checked >= 1_000_000
    assert bad == 0, first


def test_unclamped_price_at_every_value_of_whole_win_ranges(L):
    """every v of the range, for the cfg2-like law and for bids that win everything"""
    bid_c = np.array([1, 2, 57, 250, 10_000, 1_000_000_000, 1_000_000_000], np.int32)
    loc = np.array([0.0, 0.01, 0.6, 2.0, 1.5, 5.0, 9.0e6], np.float32)
    scale = np.array([0.004, 0.3, 0.25, 1.0, 3.0, 2.0, 4.0e5], np.float32)
    bad, checked, first = proven(L, bid_c, loc, scale, 0.3, exhaustive_below=1 << 24, ends=0, samples=0)
    assert checked >= 3 * (1 << 24)                                      # (the large bids win the whole 24-bit range)
    assert bad == 0, first


@pytest.mark.parametrize("bid_c", [1, 1_000_000_000])
def test_unclamped_price_with_adversarial_laws(L, bid_c):
    """bids of 1 cent and of 1e9 cents against NaN, infinite, zero, huge and tiny parameters: a NaN or out-of-range price is
    never inside a win range, so nothing may differ there (and most of these ranges are empty or whole)"""
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0e-30, 1.0, 9.99e6, 1.0e7, 1.0001e7, 3.0e7, 1.0e30, -1.0e7, -1.0e30], np.float32)
    loc, scale = (a.ravel() for a in np.meshgrid(special, special, indexing="ij"))
    for bctr in (0.0, 0.37, 1.0, np.nan):
        bad, checked, first = proven(L, np.full(loc.size, bid_c, np.int32), loc, scale, bctr, exhaustive_below=4096, ends=64, samples=64)
        assert bad == 0, (bctr, first)
    # scale 0 with the price just inside and just outside the bid: the range is everything or nothing
    locs = np.array([(bid_c - 1) / 100.0, bid_c / 100.0, (bid_c + 1) / 100.0], np.float32)
    bad, checked, first = proven(L, np.full(3, bid_c, np.int32), locs, 0.0, 0.5, exhaustive_below=0, ends=256, samples=256)
    assert bad == 0, first


def test_no_win_range_where_the_clamp_acts(L):
    """a price law far above 1e9 cents, where the clamp acts at every value: the largest bid has no win range there"""
    bad, checked, first = proven(L, np.array([1_000_000_000], np.int32), 3.0e7, 1.0, 0.5, exhaustive_below=0, ends=8, samples=8)
    assert checked == 0 and bad == 0                                     # no win range, nothing to compare
