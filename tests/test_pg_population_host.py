"""Learner populations on the host: adc_pg_pop_config_check, that every new entry point is exported by the library and declared
in include/adcraft_engine.h, and what PGPopulationTrainer refuses before it touches an engine.  No device is needed.  None of
these symbols exists before this feature: every test here fails on the parent commit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import mlp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = (
    "adc_engine_mlp_learners", "adc_engine_mlp_set_learner_layer", "adc_engine_mlp_set_learner_log_std", "adc_engine_mlp_get_learner_params",
    "adc_pg_pop_config_check", "adc_engine_pg_pop_init", "adc_engine_pg_pop_advantages", "adc_engine_pg_pop_advantages_fetch", "adc_engine_pg_pop_minibatch",
    "adc_engine_pg_pop_update", "adc_engine_pg_pop_state_get", "adc_engine_pg_pop_state_set", "adc_engine_pg_pop_set_config",
    "adc_engine_pg_pop_copy")


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _configs(*options):
    from adcraft_amd import _ffi
    from adcraft_amd.engine import StepEngine
    built = [StepEngine.pg_config(**o) for o in options]
    return (_ffi.PGConfig * len(built))(*built)


def _check(lib, arr, count, num_envs, members):
    msg = C.c_char_p()
    rc = lib.adc_pg_pop_config_check(arr, count, num_envs, members, C.byref(msg))
    return rc, msg.value


MIXED = (dict(eps_clip=0.2, normalize_advantages=True, lr=3e-4),                                             # PPO
         dict(eps_clip=0.0, lam=1.0, normalize_advantages=False, lr=7e-4, gamma=0.9, ent_coef=0.01),        # A2C
         dict(optimiser="sgd", lr=0.01, max_grad_norm=0.0, reward_scale=0.05, vf_coef=1.0))                 # SGD


def test_a_mixed_array_is_accepted(lib):
    arr = _configs(*MIXED)
    assert _check(lib, arr, 3, 480, 3) == (0, None)
    assert _check(lib, arr, 1, 480, 3) == (0, None)                # one configuration shared by all
    assert _check(lib, arr, 1, 480, 1) == (0, None)
    arr = _configs(*(dict(o, minibatch_envs=80) for o in MIXED))
    assert _check(lib, arr, 3, 480, 3) == (0, None)                # 80 divides 480 / 3
    assert _check(lib, arr, 3, 240, 3) == (0, None)                # ... and is all of 240 / 3
    # without a message pointer
    assert lib.adc_pg_pop_config_check(arr, 3, 480, 3, None) == 0


def test_each_refusal_gives_a_message(lib):
    from adcraft_amd import _ffi
    bad = _ffi.ADC_EINVAL
    # unequal minibatch_envs
    arr = _configs(dict(MIXED[0], minibatch_envs=80), dict(MIXED[1], minibatch_envs=40), dict(MIXED[2], minibatch_envs=80))
    rc, msg = _check(lib, arr, 3, 480, 3)
    assert rc == bad and b"equal" in msg
    arr = _configs(dict(MIXED[0], minibatch_envs=0), dict(MIXED[1], minibatch_envs=160), MIXED[2])
    rc, msg = _check(lib, arr, 3, 480, 3)
    assert rc == bad and b"equal" in msg                           # (0 and N / M name the same minibatch, but are not equal fields)
    # a minibatch_envs that does not divide N / M, or exceeds it
    for mb in (60, 320, 480):
        arr = _configs(*(dict(o, minibatch_envs=mb) for o in MIXED))
        rc, msg = _check(lib, arr, 3, 480, 3)
        assert rc == bad and b"divide" in msg, mb
    # members not dividing num_envs; no members; no envs
    arr = _configs(*MIXED)
    for num_envs, members in ((481, 3), (480, 7), (480, 0), (480, -1), (0, 3)):
        rc, msg = _check(lib, arr, 3 if members == 3 else 1, num_envs, members)
        assert rc == bad and b"members" in msg, (num_envs, members)
    # a count that is neither 1 nor M
    for count in (0, 2, 4, -1):
        rc, msg = _check(lib, arr, count, 480, 3)
        assert rc == bad and b"count" in msg, count
    # any configuration the solo check refuses, wherever it stands, with the solo check's own message
    for at in range(3):
        for field, value in (("gamma", 1.5), ("reward_scale", 0.0), ("lr", -1.0), ("optimiser", 7), ("struct_size", 4)):
            arr = _configs(*MIXED)
            setattr(arr[at], field, value)
            solo = C.c_char_p()
            assert lib.adc_pg_config_check(C.byref(arr[at]), C.byref(solo)) == bad
            rc, msg = _check(lib, arr, 3, 480, 3)
            assert rc == bad and msg == solo.value, (at, field)
    # with a shared configuration only the first is looked at
    arr = _configs(*MIXED)
    arr[1].gamma = 1.5
    assert _check(lib, arr, 1, 480, 3) == (0, None)
    rc, msg = _check(lib, None, 1, 480, 3)
    assert rc == bad and msg


def test_every_new_entry_point_is_exported_and_declared(lib):
    with open(os.path.join(ROOT, "include", "adcraft_engine.h")) as f:
        header = f.read()
    for name in NEW_ENTRY_POINTS:
        assert getattr(lib, name) is not None                      # (AttributeError: the library does not export it)
        assert getattr(lib, name).argtypes is not None, f"{name} has no signature in _ffi"
        assert re.search(r"^int " + name + r"\(", header, re.M), f"{name} is not declared in include/adcraft_engine.h"


def test_python_surface():
    from adcraft_amd.engine import ShardedStepEngine, StepEngine
    for name in ("mlp_learners", "mlp_set_learner", "mlp_learner_params", "pg_pop_init", "pg_pop_advantages", "pg_pop_minibatch", "pg_pop_update",
                 "pg_pop_state", "pg_pop_set_config", "pg_pop_copy"):
        assert callable(getattr(StepEngine, name)), name
    sharded = object.__new__(ShardedStepEngine)
    for name in ("mlp_learners", "pg_pop_init", "pg_pop_update"):
        with pytest.raises(NotImplementedError, match="engine_shards=1"):
            getattr(sharded, name)
    arr, count = StepEngine.pg_pop_configs([dict(lr=1e-3), dict(lr=1e-4, optimiser="sgd")], 8, 2)
    assert count == 2 and abs(arr[1].lr - 1e-4) < 1e-10
    arr, count = StepEngine.pg_pop_configs(dict(lr=1e-3), 8, 2)
    assert count == 1
    with pytest.raises(ValueError, match="count"):
        StepEngine.pg_pop_configs([dict(), dict(), dict()], 8, 2)
    with pytest.raises(ValueError, match="equal"):
        StepEngine.pg_pop_configs([dict(minibatch_envs=2), dict(minibatch_envs=4)], 8, 2)


class _Untouchable:
    """an engine that fails the test when anything of it is used"""

    def __getattr__(self, name):
        raise AssertionError(f"PGPopulationTrainer touched the engine ({name}) before refusing")


def test_the_trainer_refuses_before_touching_an_engine():
    from adcraft_amd.baselines.pg_trainer import PGPopulationTrainer, a2c, ppo
    rng = np.random.default_rng(5)
    K = 3
    a = R.random_policy(rng, K, (20, 9), value=True, normalize=True)
    b = R.random_policy(rng, K, (20, 9), value=True, normalize=True)
    other_hidden = R.random_policy(rng, K, (20, 8), value=True, normalize=True)
    no_value = R.random_policy(rng, K, (20, 9), value=False, normalize=True)
    two_heads = R.random_policy(rng, K, (20, 9), two_heads=True, value=True, normalize=True)
    for p in (b, other_hidden, no_value, two_heads):               # (the normalisation is shared by all members)
        p.shift, p.scale = a.shift, a.scale
    other_norm = R.random_policy(rng, K, (20, 9), value=True, normalize=True)
    e = _Untouchable()
    with pytest.raises(ValueError, match="normalisation"):
        PGPopulationTrainer(e, [a, other_norm], 7, [ppo()])
    for pols in ([a, other_hidden], [a, b, no_value], [two_heads, a]):
        with pytest.raises(ValueError, match="equal shapes"):
            PGPopulationTrainer(e, pols, 7, [ppo()] * len(pols))
    # a wrong number of configurations
    with pytest.raises(ValueError, match="configurations"):
        PGPopulationTrainer(e, [a, b, a], 7, [ppo(), a2c(minibatches=4, epochs=10)])
    with pytest.raises(ValueError, match="configurations"):
        PGPopulationTrainer(e, [a, b], 7, [ppo(), ppo(), ppo()])
    with pytest.raises(ValueError):
        PGPopulationTrainer(e, [a, b], 7, [])
    with pytest.raises(ValueError):
        PGPopulationTrainer(e, [], 7, [ppo()])
    # members that would not move in lock-step
    with pytest.raises(ValueError, match="lock-step"):
        PGPopulationTrainer(e, [a, b], 7, [ppo(), a2c()])
