"""GPU: the IMPLICIT bid curves and ideal profit (k_ideal_profit, get_implicit_kw_bid_cpc_impressions, experiment_metrics.py:20-61)
in all three of its output modes - the maximum (adc_engine_ideal_profit), packed curve points (adc_engine_bid_curves_build / _fetch,
the per-step ideal on them, the oracle bidder) and ir / cpc arrays (adc_bid_curves_from_samples) - against the estimator written out
exactly (helpers.exact_implicit_curve) on the very METRIC samples the device draws, regenerated on the CPU by the oracle.  Sample
counts, grids and competitor laws at the edges of the kernel's bins, lanes, prefix sums and contender lists."""
import ctypes as C

import numpy as np
import pytest

from oracle import capi as orc, ref_numpy as rn
from tests import helpers as H

pytestmark = pytest.mark.gpu

NOTEBOOK = np.arange(0.01, 3.00, 0.01)
TOP_CENTS = 2046                    # the highest bid the IMPLICIT estimator keeps (include/adcraft_engine.h)


def _grids():
    rng = np.random.default_rng(7)
    return {
        "notebook": NOTEBOOK,                                       # non-decimal doubles: "0.10" is 0.09999999999999999
        "notebook_round": np.round(NOTEBOOK, 2),
        "coarse": np.arange(0.05, 2.0, 0.05),
        "subcent": np.arange(0.002, 2.5, 0.002),                    # 1249 points: the whole grid, no contender lists
        "one": np.array([0.75]),
        "n256": np.linspace(0.02, 4.0, 256),                        # cont_cap and kContenderLines edges
        "n257": np.linspace(0.02, 4.0, 257),
        "n304": np.linspace(0.02, 4.0, 304),
        "n305": np.linspace(0.02, 4.0, 305),
        "duplicated": np.repeat(np.arange(0.1, 2.0, 0.1), 3),
        "descending": NOTEBOOK[::-1].copy(),
        "shuffled": rng.permutation(NOTEBOOK),
        "nonpositive": np.concatenate([[0.0, -0.01, -0.05], np.arange(0.01, 1.5, 0.01), [-0.01, 0.0]]),
        "top1022": np.append(np.arange(0.05, 10.2, 0.05), 10.22),
        "top1023": np.append(np.arange(0.05, 10.2, 0.05), 10.23),
        "top_ceiling": np.append(np.arange(0.1, 20.4, 0.1), TOP_CENTS / 100.0),
    }


GRIDS = _grids()
# (loc, scale) of the competitor law (planes 2 and 3) per keyword column; None = H.implicit_params' default law
LAWS = [None, (12.0, 2.0), (10.2, 0.03), (1.0, 1e-4), (0.0, 0.01), (0.0, 2.0e7), (40.0, 1.0), (0.004, 0.001),
        (20.0, 1.5), (0.5, 0.3), None, (2.5, 4.0), None, (5.0, 0.0)]
SKIPS = 4                           # the last columns: no volume, no clicks, no margin, a negative margin


def _planes(N, seed):
    K = len(LAWS) + SKIPS + 1       # (19: N * K is no multiple of 32)
    p = H.implicit_params(N, K, seed=seed)
    for k, law in enumerate(LAWS):
        if law is not None:
            p[2, :, k], p[3, :, k] = law
            p[6, :, k] = np.float32(2.0 * min(law[0], 30.0) + 1.0)      # a margin the curve can be profitable under
    s = len(LAWS)
    p[0, :, s] = 0.0
    p[4, :, s + 1] = 0.0
    p[5, :, s + 2] = 0.0
    p[6, :, s + 3] = -1.0
    return p


def _engine(amd, planes, seed):
    e = amd.StepEngine(planes.shape[1], planes.shape[2], seed=seed)
    e.set_all_params(planes)
    e.reset()
    return e


def _samples(keys, ticks, planes, env, k, n):
    return orc.metric_competitor_cents(int(keys[env]), int(ticks[env]), k, n, planes[2, env, k], planes[3, env, k])


def _from_samples(cents, grid):
    from adcraft_amd import _ffi
    s = np.ascontiguousarray(cents, dtype=np.int32)
    g = np.ascontiguousarray(grid, dtype=np.float64)
    ir, cpc = np.zeros(g.size), np.zeros(g.size)
    _ffi.check(_ffi.lib().adc_bid_curves_from_samples(0, s.ctypes.data, s.size, g.ctypes.data, g.size, ir.ctypes.data, cpc.ctypes.data))
    return ir, cpc


def _run(amd, monkeypatch, planes, n, grid, seed, keywords=None, tape=3):
    """every output mode on one keyword set; each compared with the exact estimator on the regenerated samples"""
    runs = {}
    for full in ("1", "0"):
        monkeypatch.setenv("ADCRAFT_IDEAL_FULL_SCAN", full)
        e = _engine(amd, planes, seed)
        keys, ticks = e.get_rng_state()
        ideal = e.ideal_profit(n, grid)
        e.bid_curves_build(n, grid)
        ir, cpc = e.bid_curves_fetch()
        step_ideal, best = e.ideal_step()
        e.policy_oracle(123.0)
        bids, _ = e.get_actions()
        assert np.array_equal(e.get_rng_state()[0], keys) and np.array_equal(e.get_rng_state()[1], ticks)
        e.close()
        runs[full] = (step_ideal, best, bids)
    N, K = planes.shape[1:]
    todo = [(env, k) for env in range(N) for k in range(K)] if keywords is None else keywords
    for j, (env, k) in enumerate(todo):
        cents = _samples(keys, ticks, planes, env, k, n)
        xir, xcpc = H.exact_implicit_curve(cents, grid)
        _, xideal, xbest = H.exact_profit(planes, env, k, xir, xcpc)
        where = (env, k, n)
        assert np.array_equal(ir[env, k], xir), where
        assert np.array_equal(cpc[env, k], xcpc), (where, np.flatnonzero(cpc[env, k] != xcpc)[:5])
        assert ideal[env, k] == xideal, (where, ideal[env, k], xideal)
        for full, (si, sb, bids) in runs.items():
            assert si[env, k] == xideal, (where, full, si[env, k], xideal)
            assert sb[env, k] == xbest, (where, full, sb[env, k], xbest)
            assert bids[env, k] == np.float32(max(np.rint(grid[xbest] * 100.0), 1.0) / 100.0), (where, full)
        rir, rcpc = rn.implicit_bid_cpc_impressions(cents.astype(np.float64).reshape(1, -1) / 100.0, grid)
        assert np.array_equal(xir, rir), where
        np.testing.assert_allclose(xcpc, rcpc, rtol=1e-9, err_msg=str(where))
        if j < tape:
            tir, tcpc = _from_samples(cents, grid)
            assert np.array_equal(tir, xir) and np.array_equal(tcpc, xcpc), where


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


@pytest.mark.parametrize("grid_name", ["notebook", "shuffled", "top_ceiling"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, 2047, 2048, 2049, 4096])
def test_sample_counts(amd, monkeypatch, n, grid_name):
    _run(amd, monkeypatch, _planes(2, seed=40 + n), n, GRIDS[grid_name], seed=3 + n)


@pytest.mark.parametrize("n", [2048, 65])
@pytest.mark.parametrize("grid_name", [g for g in GRIDS if g not in ("notebook", "shuffled", "top_ceiling")])
def test_grids(amd, monkeypatch, grid_name, n):
    _run(amd, monkeypatch, _planes(2, seed=7), n, GRIDS[grid_name], seed=11)


@pytest.mark.parametrize("grid_name", ["notebook", "top_ceiling"])
def test_prefix_sums_at_the_sample_bound(amd, monkeypatch, grid_name):
    """2^20 samples massed at the top kept bin: the 32-bit prefix sums at their largest"""
    n = 1 << 20
    p = H.implicit_params(1, 3, seed=5)
    p[2, 0, 1], p[3, 0, 1] = TOP_CENTS / 100.0 - 0.005, 0.004
    p[2, 0, 2], p[3, 0, 2] = 2.9, 0.02
    p[6, 0, 1:] = 50.0
    _run(amd, monkeypatch, p, n, GRIDS[grid_name], seed=2)


@pytest.mark.parametrize("N,K", [(1, 1), (1, 5), (3, 1111)])
def test_keyword_shapes(amd, monkeypatch, N, K):
    """a wavefront walks several keywords: tables left over from the previous keyword would show.  Checked: the first and last
    64 keywords (the first and last workgroup's chunk) and a seeded sample of the rest"""
    p = H.implicit_params(N, K, seed=N * K)
    rng = np.random.default_rng(K)
    p[2] = np.where(rng.random((N, K)) < 0.3, np.float32(11.0), p[2])      # some keywords straddle 1023 cents
    p[3] = np.where(rng.random((N, K)) < 0.1, np.float32(1e-4), p[3])
    p[6] = np.where(p[2] > 10.0, np.float32(25.0), p[6])
    p[0] = np.where(rng.random((N, K)) < 0.1, np.float32(0.0), p[0])
    nk = N * K
    flat = sorted(set(range(min(64, nk))) | set(range(max(0, nk - 64), nk)) | set(rng.choice(nk, min(nk, 200), replace=False).tolist()))
    kws = [(i // K, i % K) for i in flat]
    for n, grid in ((2048, NOTEBOOK), (65, GRIDS["top1023"])):
        _run(amd, monkeypatch, p, n, grid, seed=13, keywords=kws)


def test_refusals(amd):
    """bids outside what the estimator keeps, non-finite bids, sample counts past the prefix sums' bound: refused, never clamped"""
    e = _engine(amd, H.implicit_params(1, 4, seed=1), seed=1)
    bad_grids = [np.append(NOTEBOOK, (TOP_CENTS + 1) / 100.0), np.append(NOTEBOOK, 30.0), np.append(NOTEBOOK, np.nan),
                 np.append(NOTEBOOK, np.inf), np.append(NOTEBOOK, -np.inf)]
    for g in bad_grids:
        with pytest.raises(ValueError):
            e.ideal_profit(2048, g)
        with pytest.raises(ValueError):
            e.bid_curves_build(2048, g)
        with pytest.raises(ValueError):
            _from_samples(np.arange(100, dtype=np.int32), g)
    for f in (e.ideal_profit, e.bid_curves_build):
        with pytest.raises(ValueError, match="2\\^20"):
            f((1 << 20) + 1, NOTEBOOK)
    with pytest.raises(ValueError, match="negative"):
        _from_samples(np.array([5, -1, 7], dtype=np.int32), NOTEBOOK)
    e.close()


def test_tape_samples_at_the_int32_edges(amd):
    """caller samples up to 2^31 - 1 cents: the cpc numerator (sum + next larger sample) passes 2^31"""
    big = np.int32(2**31 - 1)
    for cents in (np.array([3, 99, 150, 150, 2000, big, big, 1_000_000_000], dtype=np.int32),
                  np.array([0] * 5 + [TOP_CENTS] * 1000 + [big], dtype=np.int32),
                  np.full(7, big, dtype=np.int32)):
        for grid in (NOTEBOOK, GRIDS["top_ceiling"], GRIDS["nonpositive"]):
            ir, cpc = _from_samples(cents, grid)
            xir, xcpc = H.exact_implicit_curve(cents, grid)
            assert np.array_equal(ir, xir) and np.array_equal(cpc, xcpc)
