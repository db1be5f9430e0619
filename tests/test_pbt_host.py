"""-m "not gpu": the population-based training scheduler's host twins (adc_pbt_fitness_host, adc_pbt_plan_host,
adc_pbt_explore_host) against the numpy restatement tests/pbt_ref.py, bit for bit, and every refusal of adc_pbt_config_check.
The symbols do not exist before this feature: every test here fails on the parent commit."""
import ctypes as C

import numpy as np
import pytest

from tests import pbt_ref as B

F = np.float32


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _config(kind="pg", members=8, replace_count=2, **kw):
    from adcraft_amd.engine import StepEngine
    return StepEngine.pbt_config(kind, members, replace_count, **kw)


def test_fitness_twin_equals_the_restatement_bit_for_bit(lib):
    rng = np.random.default_rng(7)
    for T, N, M in ((1, 1, 1), (1, 6, 3), (6, 12, 6), (5, 12, 12), (7, 15, 3), (33, 70, 7)):
        r = (rng.standard_normal((T, N)) * 10.0 ** rng.integers(-30, 30, (T, N))).astype(F)
        r[rng.random((T, N)) < 0.2] = F(-0.0)
        r.flat[0] = F(-0.0)
        assert _same(B.twin_fitness(lib, r, M), B.fitness(r, M)), (T, N, M)
    # an all -0 record: the chain starts from +0
    z = np.full((3, 4), -0.0, F)
    got = B.twin_fitness(lib, z, 2)
    assert _same(got, B.fitness(z, 2)) and not np.signbit(got).any()
    # cancellation and overflow in float64 order: the order of the chain matters and is the stated one
    r = np.array([[3e38, 1.0], [-3e38, 1e-30], [1.0, -1.0]], F)
    assert _same(B.twin_fitness(lib, r, 1), B.fitness(r, 1))
    assert _same(B.twin_fitness(lib, r, 2), B.fitness(r, 2))


def _fitness_cases(M, rng):
    base = rng.standard_normal(M)
    ties = base.copy()
    ties[: M // 2 + 1] = 1.5
    odd = base.copy()
    odd[0] = np.nan
    odd[-1] = np.inf
    if M >= 3:
        odd[1] = -np.inf
    zeros = np.zeros(M)
    zeros[::2] = -0.0
    nans = np.full(M, np.nan)
    if M >= 3:
        nans[1] = 0.25
    return dict(plain=base, ties=ties, odd=odd, zeros=zeros, nans=nans)


@pytest.mark.parametrize("M", [2, 3, 8, 17])
def test_plan_twin_equals_the_restatement_for_every_legal_q(lib, M):
    rng = np.random.default_rng(100 + M)
    seed = 0xC0FFEE + M
    for name, fit in _fitness_cases(M, rng).items():
        for q in range(1, M // 2 + 1):
            c = _config(members=M, replace_count=q)
            s, rank, src, bits = B.twin_plan(lib, c, seed, 0, fit, np.zeros(M))
            r_rank, r_src, r_bits = B.plan(seed, 0, q, fit)
            assert _same(s, np.asarray(fit, np.float64)), "round 0: s = f"
            assert _same(rank, r_rank) and _same(src, r_src) and _same(bits, r_bits), (name, q)
            assert sorted(rank) == list(range(M))
            dst = {m for m in range(M) if src[m] >= 0}
            assert len(dst) == q and dst == {m for m in range(M) if rank[m] < q}
            assert all(rank[src[m]] >= M - q for m in dst), "every donor lies in the top q"
            assert not dst & {int(src[m]) for m in dst}, "no destination is a source"
            # the same inputs and round: the same plan
            again = B.twin_plan(lib, c, seed, 0, fit, np.zeros(M))
            assert all(_same(a, b) for a, b in zip(again, (s, rank, src, bits)))
    # NaN below every number, several NaNs by index; +-0 tie by index
    fit = _fitness_cases(M, rng)["nans"]
    rank = B.twin_plan(lib, _config(members=M, replace_count=1), seed, 0, fit, np.zeros(M))[1]
    nan_members = [m for m in range(M) if np.isnan(fit[m])]
    assert [rank[m] for m in nan_members] == list(range(len(nan_members)))
    rank = B.twin_plan(lib, _config(members=M, replace_count=1), seed, 0, _fitness_cases(M, rng)["zeros"], np.zeros(M))[1]
    assert list(rank) == list(range(M))


def test_another_round_gives_another_draw(lib):
    M, q, seed = 17, 8, 99
    fit = np.arange(M, dtype=np.float64)
    c = _config(members=M, replace_count=q)
    plans = [B.twin_plan(lib, c, seed, r, fit, fit) for r in range(4)]
    for r, (s, rank, src, bits) in enumerate(plans):
        r_rank, r_src, r_bits = B.plan(seed, r, q, fit)
        assert _same(src, r_src) and _same(bits, r_bits) and _same(rank, r_rank)
    assert len({tuple(p[3]) for p in plans}) == 4 and len({tuple(p[2]) for p in plans}) > 1
    other = B.twin_plan(lib, c, seed + 1, 0, fit, fit)
    assert not _same(other[3], plans[0][3]), "another seed: another draw"


def test_ema_over_three_rounds(lib):
    M, seed = 8, 5
    rng = np.random.default_rng(3)
    for ema in (0.0, 0.3, 0.9):
        c = _config(members=M, replace_count=2, fitness_ema=ema)
        cfg = B.config_dict(c)
        s_twin, s_ref = np.zeros(M), np.zeros(M)
        for r in range(3):
            fit = rng.standard_normal(M) * 100
            s_twin, rank, src, bits = B.twin_plan(lib, c, seed, r, fit, s_twin)
            s_ref = B.smooth(cfg["fitness_ema"], s_ref, fit, r == 0)
            assert _same(s_twin, s_ref), (ema, r)
            assert _same(src, B.plan(seed, r, 2, s_ref)[1])
            if ema == 0.0 or r == 0:
                assert _same(s_twin, fit)
        assert ema == 0.0 or not _same(s_twin, fit)


@pytest.mark.parametrize("kind", ["pg", "td3"])
def test_explore_every_id_both_factors_and_both_bounds(lib, kind):
    ids = B.PG_IDS if kind == "pg" else B.TD3_IDS
    k = B.PG if kind == "pg" else B.TD3
    bounds = {"lr": (1e-5, 1e-2), "ent_coef": (0.0, 0.1), "eps_clip": (0.05, 0.4), "vf_coef": (0.1, 2.0), "actor_lr": (1e-5, 1e-2),
              "critic_lr": (1e-5, 1e-2), "target_noise": (0.0, 0.5), "tau": (1e-3, 0.5), "sigma": (0.01, 1.0)}
    own = np.array([0.123, 0.5, 0.3, 0.7, -1.0, 9.0, 9.0, 9.0], F)
    for h, name in enumerate(ids):
        c = _config(kind, tuned=(name,), bounds=bounds, factors=(0.8, 1.25))
        cfg = B.config_dict(c)
        lo, hi = cfg["lo"][h], cfg["hi"][h]
        span = [lo, hi, np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf)), F(lo * F(1.2)), F(hi * F(0.9)), F(lo - F(3)), F(hi + F(3)),
                F((lo + hi) / 2), F(0.0)]
        for v in span:
            donor = np.array([7.0] * 8, F)
            donor[h] = v
            for bits in (0, 1 << h, 0xFFFFFFFF, 0xFFFFFFFF ^ (1 << h)):
                got, ref = B.twin_explore(lib, c, k, bits, donor, own), B.explore(cfg, k, bits, donor, own)
                assert _same(got, ref), (name, v, bits)
                assert lo <= got[h] <= hi
                others = [i for i in range(8) if i != h]
                assert _same(got[others], own[others]), "ids outside the mask keep the member's own value"
        # both factors are reached, and differ, inside the bounds
        mid = np.array([F((lo + hi) / 2)] * 8, F)
        down, up = B.twin_explore(lib, c, k, 0, mid, own)[h], B.twin_explore(lib, c, k, 1 << h, mid, own)[h]
        assert down < mid[h] < up
        if name == "sigma":
            assert _same(down, F(mid[h] + F(np.log(0.8)))) and _same(up, F(mid[h] + F(np.log(1.25))))
        else:
            assert _same(down, F(mid[h] * F(0.8))) and _same(up, F(mid[h] * F(1.25)))
    # all ids at once
    c = _config(kind, tuned=ids, bounds=bounds)
    donor = np.array([3e-4, 1e-3, 0.2, 0.01, -2.0, 0, 0, 0], F)
    for bits in range(32):
        assert _same(B.twin_explore(lib, c, k, bits, donor, own), B.explore(B.config_dict(c), k, bits, donor, own))


def test_whole_round_of_the_restatement_is_consistent():
    """the restatement's own round: a replaced member carries its donor's s, kept members their own values"""
    c = _config("pg", tuned=("lr",), bounds={"lr": (1e-5, 1e-2)}, fitness_ema=0.5)
    cfg = B.config_dict(c)
    hp = np.zeros((8, 8), F)
    hp[:, 0] = np.logspace(-5, -2, 8).astype(F)
    state = dict(round=0, smoothed=np.zeros(8))
    for r in range(3):
        fit = np.random.default_rng(r).standard_normal(8)
        state, res = B.round_(cfg, B.PG, 11, state, fit, hp)
        for m in range(8):
            if res["src"][m] >= 0:
                assert res["smoothed"][m] == res["smoothed"][res["src"][m]]
            else:
                assert _same(res["hp"][m], hp[m])
        hp = res["hp"]
    assert state["round"] == 3


def _check(lib, c, members, kind):
    msg = C.c_char_p()
    rc = lib.adc_pbt_config_check(C.byref(c) if c is not None else None, members, kind, C.byref(msg))
    return rc, (msg.value or b"").decode()


def test_config_check_refusals(lib):
    from adcraft_amd import _ffi

    def good(kind="pg"):
        tuned, bounds = (("lr", "eps_clip"), {"lr": (1e-5, 1e-2), "eps_clip": (0.05, 0.4)}) if kind == "pg" else \
            (("tau", "sigma", "target_noise"), {"tau": (1e-3, 0.5), "sigma": (0.01, 1.0), "target_noise": (0.0, 0.5)})
        return _config(kind, members=8, replace_count=2, tuned=tuned, bounds=bounds)

    assert _check(lib, good(), 8, B.PG) == (0, "") and _check(lib, good("td3"), 8, B.TD3) == (0, "")
    assert _check(lib, good(), 4, B.PG)[0] == 0 and _check(lib, good(), 5, B.PG)[0] == 0
    assert _check(lib, None, 8, B.PG)[0] == _ffi.ADC_EINVAL

    def refused(change, members=8, kind="pg", word=""):
        c = good(kind)
        change(c)
        rc, msg = _check(lib, c, members, B.PG if kind == "pg" else B.TD3)
        assert rc == _ffi.ADC_EINVAL and word in msg, (rc, msg, word)

    refused(lambda c: setattr(c, "struct_size", 8), word="struct_size")
    refused(lambda c: None, members=1, word="at least 2")
    refused(lambda c: None, members=3, word="replace_count")               # q = 2 > 3 / 2
    refused(lambda c: setattr(c, "replace_count", 0), word="replace_count")
    refused(lambda c: setattr(c, "replace_count", 5), word="replace_count")
    for ema in (-0.1, 1.0, float("nan")):
        refused(lambda c: setattr(c, "fitness_ema", ema), word="fitness_ema")
    for f in (0.0, -1.0, float("inf"), float("nan")):
        refused(lambda c: setattr(c, "factor_lo", f), word="factor")
        refused(lambda c: setattr(c, "factor_hi", f), word="factor")
    for f in (float("inf"), float("-inf"), float("nan")):
        refused(lambda c: setattr(c, "log_factor_lo", f), word="log_factor")
        refused(lambda c: setattr(c, "log_factor_hi", f), word="log_factor")
    refused(lambda c: setattr(c, "tuned_mask", 1 << 4), word="tuned_mask")            # PG has four ids
    refused(lambda c: setattr(c, "tuned_mask", 1 << 5), kind="td3", word="tuned_mask")
    refused(lambda c: setattr(c, "with_ring", 1), word="ring")
    refused(lambda c: setattr(c, "with_ring", 2), kind="td3", word="with_ring")

    def bound(h, lo, hi):
        def change(c):
            c.tuned_mask |= 1 << h
            c.lo[h], c.hi[h] = lo, hi
        return change
    refused(bound(0, 1e-2, 1e-5), word="lo <= hi")
    refused(bound(0, float("nan"), 1e-2), word="lo")
    refused(bound(0, 1e-5, float("inf")), word="finite")
    refused(bound(0, -1e-5, 1e-2), word="at least 0")
    refused(bound(1, -0.5, 0.1), word="at least 0")
    refused(bound(3, -0.5, 0.1), word="at least 0")
    refused(bound(2, 0.05, 1.0), word="eps_clip")
    assert _check(lib, (lambda c: (bound(2, -1.0, 0.5)(c), c)[1])(good()), 8, B.PG)[0] == 0, "eps_clip <= 0 is legal: no clip"
    refused(bound(3, 0.0, 0.5), kind="td3", word="tau")
    refused(bound(3, 1e-3, 1.5), kind="td3", word="tau")
    refused(bound(2, -0.1, 0.5), kind="td3", word="at least 0")
    refused(bound(4, 0.0, -1.0), kind="td3", word="lo <= hi")
    assert _check(lib, (lambda c: (bound(4, -5.0, -1.0)(c), c)[1])(good("td3")), 8, B.TD3)[0] == 0, "sigma's bounds are logarithms: negative is legal"
    # an untuned id's bounds are not read
    c = good()
    c.lo[3], c.hi[3] = 5.0, -5.0
    assert _check(lib, c, 8, B.PG)[0] == 0
    # a bad kind
    rc, msg = _check(lib, good(), 8, 2)
    assert rc == _ffi.ADC_EINVAL and "kind" in msg


def test_python_config_fills_the_log_factors_and_sigma_bounds():
    c = _config("td3", tuned=("sigma",), bounds={"sigma": (0.01, 1.0)}, factors=(0.5, 2.0))
    assert _same(F(c.log_factor_lo), F(np.log(0.5))) and _same(F(c.log_factor_hi), F(np.log(2.0)))
    assert _same(F(c.lo[4]), F(np.log(0.01))) and _same(F(c.hi[4]), F(np.log(1.0)))
    assert c.tuned_mask == 1 << 4
    with pytest.raises(ValueError):
        _config("pg", tuned=("sigma",), bounds={"sigma": (0.01, 1.0)})
    with pytest.raises(ValueError):
        _config("pg", tuned=("lr",))
    with pytest.raises(ValueError):
        _config("pg", members=8, replace_count=5)
