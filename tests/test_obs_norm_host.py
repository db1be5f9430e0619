"""The running observation normaliser on the host: the twin adc_obs_norm_host (the code the device kernels run, adc_norm.h)
against the numpy restatement tests/norm_ref.py bit for bit, its moments against float64 numpy, the invariance of the raw-space
moments under the vectors the rows were collected with, the configuration check and the Python surface.  No device is needed."""
import ctypes as C

import numpy as np
import pytest

from tests import norm_ref as NR

F, D64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _rows(rng, S, D, spread=3.0):
    """rows of mixed magnitude: a mean and a width per column"""
    mu = rng.standard_normal(D) * spread
    sd = np.exp(rng.standard_normal(D))
    return (mu + sd * rng.standard_normal((S, D))).astype(F)


def _vectors(rng, D):
    return (rng.standard_normal(D) * 2).astype(F), np.exp(rng.standard_normal(D)).astype(F)


@pytest.mark.parametrize("D", [1, 7, 127, 257])
@pytest.mark.parametrize("S", [1, 1023, 1024, 1025, 2500])
def test_twin_equals_the_restatement_from_an_empty_normaliser(lib, S, D):
    rng = np.random.default_rng(1000 * S + D)
    shift, scale = _vectors(rng, D)
    st = NR.fresh(D, shift, scale)
    x = _rows(rng, S, D)
    got, ref = NR.twin(lib, st, x), NR.update(st, x)
    assert NR.same(got, ref)
    assert got["count"] == S and np.isfinite(got["mean"]).all() and (got["scale"] > 0).all()
    assert S == 1 or not np.array_equal(got["scale"], scale), "the vectors moved"


def test_three_batches_merged(lib):
    rng = np.random.default_rng(7)
    D = 33
    got = ref = NR.fresh(D, *_vectors(rng, D))
    for i, S in enumerate((1500, 700, 2049)):
        # (each batch is collected under the vectors the update before it left, as a record's days are)
        x = _rows(rng, S, D, spread=1.0 + i)
        got, ref = NR.twin(lib, got, x), NR.update(ref, x)
        assert NR.same(got, ref), i
    assert got["count"] == 1500 + 700 + 2049
    assert (got["M2"] > 0).all()


@pytest.mark.parametrize("cap", [1000, 100000])
def test_count_cap_below_and_above_the_running_count(lib, cap):
    rng = np.random.default_rng(11 + cap)
    D = 9
    got = ref = NR.fresh(D)
    for S in (600, 600, 600):
        x = _rows(rng, S, D)
        got, ref = NR.twin(lib, got, x, count_cap=cap), NR.update(ref, x, count_cap=cap)
        assert NR.same(got, ref)
    assert got["count"] == min(cap, 1800)
    free = NR.fresh(D)
    rng = np.random.default_rng(11 + cap)
    for S in (600, 600, 600):
        free = NR.twin(lib, free, _rows(rng, S, D))
    assert NR.same(free, got) == (cap > 1800), "a cap above the count changes nothing, one below it does"


def test_constant_column_ends_at_one_over_min_std(lib):
    rng = np.random.default_rng(3)
    S, D, min_std = 1300, 5, 0.05
    x = _rows(rng, S, D)
    x[:, 2] = F(4.25)
    x[:, 4] = F(0.0)
    st = NR.fresh(D)
    got, ref = NR.twin(lib, st, x, min_std=min_std), NR.update(st, x, min_std=min_std)
    assert NR.same(got, ref)
    for j, v in ((2, 4.25), (4, 0.0)):
        assert got["scale"][j] == F(1.0 / min_std) and got["shift"][j] == F(v) and got["M2"][j] == 0.0
        assert (x[:, j] - got["shift"][j]) * got["scale"][j] == pytest.approx(0.0, abs=0)
    assert got["scale"][0] != F(1.0 / min_std)


def test_a_negative_variance_before_the_clamp(lib):
    """a column that is constant at a value whose square is not a float64: qx / S - mx * mx rounds below zero for some of them"""
    rng = np.random.default_rng(5)
    S = 1000
    vals = (1.0 + rng.random(64)).astype(F)
    x = np.broadcast_to(vals, (S, vals.size)).copy()
    x64 = x.astype(D64)
    from tests.pg_ref import csum
    mx = csum(x64) / D64(S)
    vx = csum(x64 * x64) / D64(S) - mx * mx
    assert (vx < 0).any(), "the case was meant to hold a negative variance before the clamp"
    st = NR.fresh(vals.size)
    got, ref = NR.twin(lib, st, x), NR.update(st, x)
    assert NR.same(got, ref)
    assert (got["M2"][vx < 0] == 0.0).all() and (got["scale"][vx < 0] == F(100.0)).all()


def _bound_check(state, raw, what):
    """mean and M2 / count against float64 numpy within 1e-9 relative to std and var: the rounding of a float64 sum of 3000
    terms is about 3e-13 and cancellation at |mean| <= 10 std costs at most two more decades"""
    mean, var = raw.astype(D64).mean(axis=0), raw.astype(D64).var(axis=0)
    std = np.sqrt(var)
    assert np.all(np.abs(state["mean"] - mean) <= 1e-9 * std), what
    assert np.all(np.abs(state["M2"] / state["count"] - var) <= 1e-9 * var), what


def test_moments_agree_with_float64_numpy(lib):
    rng = np.random.default_rng(21)
    D = 40
    std = np.exp(rng.standard_normal(D) * 2)
    mean = std * rng.uniform(-10, 10, D)
    raw = (mean + std * rng.standard_normal((3000, D))).astype(F)
    # one batch, and three batches merged (identity vectors: the rows are the raw data)
    st = NR.twin(lib, NR.fresh(D), raw)
    _bound_check(st, raw, "one batch")
    st = NR.fresh(D)
    for a, b in ((0, 1100), (1100, 1900), (1900, 3000)):
        ident = dict(st, shift=np.zeros(D, F), scale=np.ones(D, F))
        st = NR.twin(lib, ident, raw[a:b])
    _bound_check(st, raw, "three batches")


def test_raw_space_moments_do_not_depend_on_the_vectors(lib):
    """the same raw data through two different (shift, scale) pairs.  The shifts and scales are powers of two and small
    integers, so that (raw - shift) * scale is exact in float32 and both normalisers see the very same raw samples."""
    rng = np.random.default_rng(22)
    D = 24
    raw = np.round(rng.standard_normal((2800, D)) * 64).astype(F) / F(8)          # multiples of 1/8, |raw| < 64
    states = []
    for shift, scale in ((np.zeros(D, F), np.ones(D, F)), (rng.integers(-4, 5, D).astype(F), F(2.0) ** rng.integers(-3, 4, D).astype(F))):
        x = ((raw - shift) * scale).astype(F)
        assert np.array_equal(x.astype(D64), (raw.astype(D64) - shift) * scale), "the normalised rows were meant to be exact"
        st = NR.twin(lib, NR.fresh(D, shift, scale), x)
        _bound_check(st, raw, "against numpy")
        states.append(st)
    a, b = states
    std = np.sqrt(raw.astype(D64).var(axis=0))
    assert np.all(np.abs(a["mean"] - b["mean"]) <= 1e-9 * std)
    assert np.all(np.abs(a["M2"] / a["count"] - b["M2"] / b["count"]) <= 1e-9 * std * std)


def test_config_check_refuses_every_clause_with_a_message(lib):
    def check(c):
        msg = C.c_char_p()
        rc = lib.adc_obs_norm_config_check(None if c is None else C.byref(c), C.byref(msg))
        return rc, msg.value
    assert check(NR.config()) == (0, None)
    assert check(NR.config(min_std=1e-6, count_cap=1 << 40)) == (0, None)
    bad = [None]
    c = NR.config(); c.struct_size += 4; bad.append(c)
    for v in (0.0, -1.0, float("inf"), float("nan")):
        bad.append(NR.config(min_std=v))
    bad.append(NR.config(count_cap=-1))
    msgs = set()
    for c in bad:
        rc, msg = check(c)
        assert rc == -1 and msg, (rc, msg)
        msgs.add(msg)
    assert len(msgs) == 3, "struct_size, min_std and count_cap each have their own message"
    # the twin refuses what the check refuses, and empty batches
    x = np.zeros((4, 2), F)
    st = NR.fresh(2)
    cnt = C.c_int64(0)
    args = (C.byref(cnt), st["mean"].ctypes.data, st["M2"].ctypes.data, st["shift"].ctypes.data, st["scale"].ctypes.data)
    assert lib.adc_obs_norm_host(C.byref(NR.config(min_std=0.0)), 4, 2, x.ctypes.data, *args) == -1
    assert lib.adc_obs_norm_host(C.byref(NR.config()), 0, 2, x.ctypes.data, *args) == -1
    assert lib.adc_obs_norm_host(C.byref(NR.config()), 4, 2, None, *args) == -1


def test_python_surface():
    from adcraft_amd.engine import StepEngine
    c = StepEngine.obs_norm_config()
    assert (c.per_member, c.min_std, c.count_cap) == (0, 1e-2, 0), "the defaults are configuration: min_std 1e-2, no forgetting"
    c = StepEngine.obs_norm_config(per_member=True, min_std=0.5, count_cap=4096)
    assert (c.per_member, c.min_std, c.count_cap) == (1, 0.5, 4096)
    with pytest.raises(ValueError, match="min_std"):
        StepEngine.obs_norm_config(min_std=0.0)
    with pytest.raises(ValueError, match="count_cap"):
        StepEngine.obs_norm_config(count_cap=-5)
    import inspect
    from adcraft_amd.baselines.pg_trainer import PGPopulationTrainer, PGTrainer
    for cls in (PGTrainer, PGPopulationTrainer):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["normalize_observations"].default is False and sig["obs_norm"].default is None
