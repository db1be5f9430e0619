"""CPU: the claim k_step_implicit_fast's stage B rests on since a clicked win adds its price and its revenue with one atomic.

Soundness of the packing bound.  adc::fast_money_packs (adc_law.h; float32, as phase 1 of the kernel evaluates it per keyword) says
that V auctions at a bid of bid_c cents under the revenue law (mu, sd) keep the day's cost and the day's revenue below 2^32 cents
each, so that the two share one 64-bit accumulator.  Wherever it says so: the revenue of one conversion (adc::revenue_cents_tab, the
shared routine) stays at or below the bound r_max at the table's extreme words, and V r_max and V (bid_c - 1) are below 2^32 in exact
integer arithmetic.  A NaN or infinite law never packs.  Host build of the kernels' own adc_law.h (g++), as
tests/test_fast_dead_keywords_host.py.  (The issue's part C - stage B's integer-to-float conversions written without v_cvt - was
built, measured and taken out, profiles/pr_fast_packed_money.txt: its exactness tests went with it.)"""
import ctypes as C

import numpy as np
import pytest

from oracle import build as obuild

N_LAWS = 100_000
# the words with the largest |z| (bits 30..8 clear: p = 2^-25), both signs, with the unused low bits clear and set, and the two ends
EXTREME_WORDS = np.array([0x00000000, 0x80000000, 0x000000FF, 0x800000FF, 0xFFFFFFFF, 0x7FFFFFFF, 0x00000100, 0x80000100], np.uint32)


@pytest.fixture(scope="module")
def L():
    lib = C.CDLL(obuild.build_shims_host())
    vp = C.c_void_p
    lib.adc_fast_money_packs_host.argtypes = [C.c_int64, vp, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp]
    lib.adc_fast_money_packs_host.restype = C.c_int
    return lib


def _packs(L, V, bid, mu, sd, words=EXTREME_WORDS):
    V = np.ascontiguousarray(V, dtype=np.int32)
    bid, mu, sd = (np.ascontiguousarray(a, dtype=np.float32) for a in (bid, mu, sd))
    words = np.ascontiguousarray(words, dtype=np.uint32)
    n = V.size
    packs, bid_c, r_max = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int64)
    rev = np.zeros((n, words.size), np.int32)
    z_max = C.c_float()
    assert L.adc_fast_money_packs_host(n, V.ctypes.data, bid.ctypes.data, mu.ctypes.data, sd.ctypes.data, words.ctypes.data, words.size,
                                       packs.ctypes.data, bid_c.ctypes.data, r_max.ctypes.data, rev.ctypes.data, C.byref(z_max)) == 0
    return packs.astype(bool), bid_c, r_max, rev, float(z_max.value)


def _random_laws(rng, n):
    """mu over 1 cent .. $1e6 and sd over 1 cent .. $1e5, log-uniform, both signs, a tenth of the sds 0; bids of 1 cent .. 1e9 cents and
    volumes 1 .. 2^20, log-uniform (a fifth of the bids ordinary ones, 1 cent .. $20); 1 % of the laws with a NaN or an infinity"""
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
    return V, bid, mu, sd


def test_packing_bound_is_sound(L):
    rng = np.random.default_rng(4242)
    V, bid, mu, sd = _random_laws(rng, N_LAWS)
    words = np.concatenate([EXTREME_WORDS, rng.integers(0, 2**32, 8, dtype=np.uint64).astype(np.uint32)])
    packs, bid_c, r_max, rev, z_max = _packs(L, V, bid, mu, sd, words)
    assert 5.0 < z_max < 6.0          # -Phi^-1(2^-25) = 5.42
    # the reference predicate, in float64 and exact integers, on the inputs alone: the ranges must exercise both answers
    finite = np.isfinite(mu) & np.isfinite(sd)
    with np.errstate(invalid="ignore", over="ignore"):
        r_ref = np.where(finite, np.rint(np.maximum(np.abs(mu.astype(np.float64)) + np.abs(sd.astype(np.float64)) * z_max, 0.01) * 100.0), 1e18)
    bid_c_ref = np.clip(np.rint(bid.astype(np.float64) * 100.0), 1.0, 1.0e9).astype(np.int64)
    assert (bid_c == bid_c_ref).all()
    V64 = V.astype(np.int64)
    ref = finite & (r_ref < 1.0e9) & (V64 * np.minimum(r_ref, 1e12).astype(np.int64) < 2**32) & (V64 * (bid_c_ref - 1) < 2**32)
    print(f"reference predicate: {int(ref.sum())} of {ref.size} pack; host predicate: {int(packs.sum())}")
    assert ref.sum() >= N_LAWS // 3 and (~ref).sum() >= N_LAWS // 10
    # NaN or infinite: never
    assert (~finite).sum() > 500 and not packs[~finite].any()
    # wherever the predicate says "packs"
    p = packs
    assert (r_max[p] >= 1).all()
    assert (rev[p] <= r_max[p, None]).all() and (rev[p] >= 1).all()
    assert (V64[p] * r_max[p] < 2**32).all()
    assert (V64[p] * (bid_c[p].astype(np.int64) - 1) < 2**32).all()
    # the bound is the float32 value of |mu| + |sd| z_max in cents, not something smaller that the eight words happen to stay under
    assert (np.abs(r_max[p] - r_ref[p]) <= 1.0 + 1e-6 * r_ref[p]).all()
    # and it is not idle: what the reference admits with 10 % to spare packs (the float32 test compares with 4.0e9, 7 % below 2^32)
    spare = finite & (r_ref < 0.9e9) & (V64 * np.minimum(r_ref, 1e12).astype(np.int64) < 3.8e9) & (V64 * (bid_c_ref - 1) < 3.8e9)
    assert spare.sum() >= N_LAWS // 3 and packs[spare].all()
    assert not packs[~ref].any()


def test_packing_bound_edges(L):
    """volume 2^20 and 1, the bid at its cap, sd = 0, the largest revenue that packs at a volume, and the benchmark's own law"""
    V = np.array([2**20, 2**20, 2**20, 1, 1, 4, 5, 128, 5000, 1, 1, 1], np.int32)
    bid = np.array([38.15, 41.0, 0.5, 1.0e7, 1.0e7, 1.0e7, 1.0e7, 0.75, 50000.0, 0.5, 0.5, 0.5], np.float32)
    mu = np.array([1.0, 1.0, 45.0, 1.0, 9.0e6, 1.0, 1.0, 30.0, 30.0, np.nan, 1.0, -np.inf], np.float32)
    sd = np.array([0.0, 0.0, 0.0, 0.0, 1.0e5, 0.0, 0.0, 10.0, 10.0, 1.0, np.inf, 1.0], np.float32)
    packs, bid_c, r_max, rev, _ = _packs(L, V, bid, mu, sd)
    #        2^20 x 3814 < 4.0e9 <= 2^20 x 4099; 2^20 x 4500 cents of revenue; 1 x (1e9 - 1); 9.54e8 cents; 4 x 1e9 >= 4.0e9; 5 x 1e9
    want = [True, False, False, True, True, False, False, True, False, False, False, False]
    assert packs.tolist() == want
    assert bid_c[3] == 10**9 and r_max[9] == -1 and r_max[10] == -1 and r_max[11] == -1
