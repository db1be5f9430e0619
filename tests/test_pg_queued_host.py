"""The queued PPO / A2C update on the host: the twin adc_pg_decide_host (adc_pg_shuffle.h's pg_decide, the code k_pg_decide runs on
the device) against the numpy restatement tests/pg_queued_ref.py bit for bit on every branch of the decision, and the new
surface - the library's symbols, StepEngine's and the trainers' `queued` switches, the examples' flag.  No device is needed."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from tests import pg_queued_ref as Q
from tests import pg_shuffle_ref as S

F = np.float32
D64 = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _same(got, ref):
    return got[:3] == ref[:3] and np.array_equal(np.asarray(got[3], F).view(np.uint32), np.asarray(ref[3], F).view(np.uint32))


# ---- 1. the decision ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mgn", (0.5, 0.3, 40.0))
def test_the_clip_scale_below_at_and_above_the_bound(lib, mgn):
    """grad_norm far below, just below, equal to, just above and far above max_grad_norm, and the norm at which the quotient is
    exactly 1 (norm + 1e-6 == max_grad_norm): the twin's scale has the restatement's bits; the clip is on in all of them"""
    g = D64(F(mgn))
    edge = g - D64(1e-6)
    norms = [0.0, 1e-3 * g, np.nextafter(edge, -np.inf), edge, np.nextafter(edge, np.inf), np.nextafter(g, -np.inf), g, np.nextafter(g, np.inf),
             3.0 * g, 1e6 * g, np.inf]
    seen = set()
    for norm in norms:
        sums = Q.sums_for(0.0, 1.0, 7)
        sums[9] = D64(norm) * D64(norm)
        got, ref = Q.twin_decide(lib, mgn, 0.0, sums, 7), Q.decide(mgn, 0.0, sums, 7)
        assert _same(got, ref), (mgn, norm, got, ref)
        assert got[:3] == (1, 0, 1)
        seen.add(float(got[3]) < 1.0)
    assert seen == {True, False}
    # (the scale is the host-driven update's: pg_ref.step's quotient)
    sums = Q.sums_for(0.0, 3.0 * g, 7)
    q = D64(F(mgn)) / (np.sqrt(sums[9]) + 1e-6)
    assert Q.twin_decide(lib, mgn, 0.0, sums, 7)[3] == F(q)


def test_no_clip_without_a_bound(lib):
    """max_grad_norm = 0: the clip is off and the scale 1 whatever the norm is"""
    for norm in (0.0, 1.0, 1e30, np.inf, np.nan):
        sums = Q.sums_for(0.0, 1.0, 7)
        sums[9] = D64(norm)
        got = Q.twin_decide(lib, 0.0, 0.0, sums, 7)
        assert _same(got, Q.decide(0.0, 0.0, sums, 7)) and got[:3] == (1, 0, 0) and got[3] == F(1.0), (norm, got)


@pytest.mark.parametrize("target", (0.01, 0.3, 1e-6))
def test_the_stop_below_at_and_above_its_bound(lib, target):
    """approx_kl below, equal to and above 1.5 * f64(f32(target_kl)) (S = 8: the division is exact), and a count that is no power
    of two; the stop is adc_pg_shuffle_stop_host's on the same approx_kl, and a stopping minibatch takes no step"""
    bound = 1.5 * D64(F(target))
    for S_ in (8, 7):
        for kl, want in ((0.0, 0), (-1.0, 0), (np.nextafter(bound, -np.inf), 0), (bound, 0), (np.nextafter(bound, np.inf), 1), (10.0 * bound, 1)):
            sums = Q.sums_for(kl, 2.0, S_)
            approx = sums[3] / D64(S_)
            got, ref = Q.twin_decide(lib, 0.5, target, sums, S_), Q.decide(0.5, target, sums, S_)
            assert _same(got, ref), (target, kl, got, ref)
            assert bool(got[1]) is S.twin_stop(lib, approx, target)
            if S_ == 8:
                assert approx == kl and got[1] == want, (target, kl, got)
            if got[1]:
                assert got[2] == 0 and got[3] == F(1.0)
            else:
                assert got[2] == 1 and got[3] < F(1.0)


def test_a_zero_target_never_stops(lib):
    for kl in (0.0, 1.0, 1e30, np.inf):
        sums = Q.sums_for(kl, 2.0, 8)
        got = Q.twin_decide(lib, 0.5, 0.0, sums, 8)
        assert _same(got, Q.decide(0.5, 0.0, sums, 8)) and got[1] == 0 and got[2] == 1


def test_nan_statistics_decide_as_the_host_driven_update_does(lib):
    """a NaN approx_kl does not stop (adc_pg_shuffle_stop_host: the comparison is false) and a NaN norm gives scale 1
    (pg_clip_scale: q < 1 is false), both at once too"""
    nan = float("nan")
    for kl, norm in ((nan, 2.0), (0.0, nan), (nan, nan)):
        sums = Q.sums_for(0.0, 1.0, 7)
        sums[3], sums[9] = kl, norm
        got = Q.twin_decide(lib, 0.5, 0.01, sums, 7)
        assert _same(got, Q.decide(0.5, 0.01, sums, 7)), (kl, norm, got)
        assert got[1] == 0 and S.twin_stop(lib, sums[3] / 7.0, 0.01) is (got[1] == 1)
        assert got[2] == 1 and bool(got[3] == F(1.0)) is bool(np.isnan(norm))


def test_the_twin_refuses_bad_arguments(lib):
    from adcraft_amd.engine import StepEngine
    cfg = StepEngine.pg_config()
    sums = Q.sums_for()
    out = C.c_int32(0)
    assert lib.adc_pg_decide_host(C.byref(cfg), 0.01, sums.ctypes.data, 7, None, C.byref(out), None, None) == 0       # (outputs may be NULL)
    assert lib.adc_pg_decide_host(None, 0.01, sums.ctypes.data, 7, None, C.byref(out), None, None) != 0
    assert lib.adc_pg_decide_host(C.byref(cfg), 0.01, None, 7, None, C.byref(out), None, None) != 0
    assert lib.adc_pg_decide_host(C.byref(cfg), 0.01, sums.ctypes.data, 0, None, C.byref(out), None, None) != 0
    assert lib.adc_pg_decide_host(C.byref(cfg), -1.0, sums.ctypes.data, 7, None, C.byref(out), None, None) != 0
    assert lib.adc_pg_decide_host(C.byref(cfg), float("inf"), sums.ctypes.data, 7, None, C.byref(out), None, None) != 0


# ---- 2. the surface ----------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_exist_and_are_declared(lib):
    header = open(os.path.join(ROOT, "include", "adcraft_engine.h")).read()
    for name in ("adc_pg_decide_host", "adc_engine_pg_update_queued", "adc_engine_pg_pop_update_queued"):
        assert getattr(lib, name).restype is C.c_int, name
        assert name + "(" in header, name
    assert lib.adc_abi_version() == 5                              # (symbols were added, nothing changed)
    assert lib.adc_engine_pg_update_queued(None, 1, None) != 0 and lib.adc_engine_pg_pop_update_queued(None, 1, None) != 0


def test_the_python_layer_accepts_queued():
    from adcraft_amd.baselines import pg_trainer
    from adcraft_amd.engine import StepEngine
    for fn in (StepEngine.pg_update, StepEngine.pg_pop_update):
        assert inspect.signature(fn).parameters["queued"].default is False
    for cls in (pg_trainer.PGTrainer, pg_trainer.PGPopulationTrainer):
        assert inspect.signature(cls.__init__).parameters["queued_update"].default is False
    # the preset carries the switch only when asked: without it the configuration is what it was
    assert "queued_update" not in pg_trainer.rllib_ppo(minibatch_size=64)
    cfg = pg_trainer.rllib_ppo(minibatch_size=64, queued_update=True)
    assert cfg["queued_update"] is True and cfg["minibatch_size"] == 64
    assert {k: v for k, v in cfg.items() if k != "queued_update"} == pg_trainer.rllib_ppo(minibatch_size=64)


@pytest.mark.parametrize("script", ("train_mlp_policy_ppo.py", "sweep_ppo.py"))
def test_the_examples_offer_the_flag(script):
    text = open(os.path.join(ROOT, "examples", script)).read()
    assert '"--queued-update"' in text and "queued_update" in text
