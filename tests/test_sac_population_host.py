"""SAC learner populations on the host: adc_sac_pop_config_check, that every new entry point is exported by the library, declared
in include/adcraft_engine.h and given a signature in _ffi.py, and the Python surface.  No device is needed.  None of these symbols
exists before this feature: every test here fails on the parent commit."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = (
    "adc_engine_mlp_learners_set_squash", "adc_sac_pop_config_check", "adc_engine_sac_pop_init", "adc_engine_sac_pop_set_critic_layer",
    "adc_engine_sac_pop_sync_targets", "adc_engine_sac_pop_store", "adc_engine_sac_pop_buffer_info", "adc_engine_sac_pop_buffer_fetch",
    "adc_engine_sac_pop_buffer_load", "adc_engine_sac_pop_batch_indices", "adc_engine_sac_pop_update", "adc_engine_sac_pop_param_counts",
    "adc_engine_sac_pop_state_get", "adc_engine_sac_pop_state_set", "adc_engine_sac_pop_set_config", "adc_engine_sac_pop_copy")
K = 5


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _configs(*options):
    from adcraft_amd import _ffi
    from adcraft_amd.engine import StepEngine
    built = [StepEngine.sac_config(num_keywords=K, **o) for o in options]
    return (_ffi.SACConfig * len(built))(*built)


def _check(lib, arr, count, num_envs, members):
    msg = C.c_char_p()
    rc = lib.adc_sac_pop_config_check(arr, count, num_envs, members, C.byref(msg))
    return rc, msg.value


SHARED = dict(batch_size=7, capacity=40, critic_widths=(11, 7, 1), target_update_interval=2)
MIXED = (dict(SHARED, gamma=0.9, tau=0.05, actor_lr=1e-5, critic_lr=1e-3, alpha_lr=1e-3, init_alpha=0.3, target_entropy=-2.0, seed=0),
         dict(SHARED, gamma=0.99, tau=0.01, actor_lr=1e-3, critic_lr=3e-3, alpha_lr=0.0, init_alpha=0.7, seed=77, max_grad_norm=0.5),
         dict(SHARED, gamma=0.8, tau=1.0, optimiser="sgd", actor_lr=0.01, critic_lr=0.01, reward_scale=0.5, eps_sq=1e-5))


def test_a_shared_configuration_and_distinct_ones_are_accepted(lib):
    arr = _configs(*MIXED)
    assert _check(lib, arr, 3, 12, 3) == (0, None)
    assert _check(lib, arr, 1, 12, 3) == (0, None)                 # one configuration shared by all
    assert _check(lib, arr, 1, 12, 1) == (0, None)
    assert _check(lib, arr, 1, 65535 * 2, 65535) == (0, None)
    assert lib.adc_sac_pop_config_check(arr, 3, 12, 3, None) == 0   # without a message pointer


def test_each_refusal_gives_a_message(lib):
    from adcraft_amd import _ffi
    bad = _ffi.ADC_EINVAL
    arr = _configs(*MIXED)
    # members not dividing num_envs; no members; too many; no envs
    for num_envs, members in ((13, 3), (12, 5), (12, 0), (12, -1), (0, 3), (65536, 65536)):
        rc, msg = _check(lib, arr, 3 if members == 3 else 1, num_envs, members)
        assert rc == bad and b"members" in msg, (num_envs, members)
    # a count that is neither 1 nor M
    for count in (0, 2, 4, -1):
        rc, msg = _check(lib, arr, count, 12, 3)
        assert rc == bad and b"count" in msg, count
    # a shared field that differs, wherever it stands
    for at in (1, 2):
        for field, value, word in (("batch_size", 8, b"batch_size"), ("capacity", 41, b"capacity"),
                                   ("target_update_interval", 3, b"target_update_interval")):
            arr = _configs(*MIXED)
            setattr(arr[at], field, value)
            rc, msg = _check(lib, arr, 3, 12, 3)
            assert rc == bad and word in msg and b"equal" in msg, (at, field)
        arr = _configs(*MIXED)
        arr[at].critic_widths[0] = 12
        rc, msg = _check(lib, arr, 3, 12, 3)
        assert rc == bad and b"critic_widths" in msg and b"equal" in msg, at
        arr = _configs(*MIXED[:at], dict(MIXED[at], critic_widths=(11, 1)), *MIXED[at + 1:])
        rc, msg = _check(lib, arr, 3, 12, 3)
        assert rc == bad and b"n_critic_layers" in msg and b"equal" in msg, at
    # any configuration the solo check refuses, wherever it stands, with the solo check's own message
    for at in range(3):
        for field, value in (("gamma", 1.5), ("tau", 0.0), ("reward_scale", 0.0), ("actor_lr", -1.0), ("optimiser", 7), ("struct_size", 4),
                             ("batch_size", 0), ("init_alpha", 0.0), ("alpha_lr", -1.0), ("eps_sq", 0.0), ("target_update_interval", 0),
                             ("target_entropy", float("inf"))):
            arr = _configs(*MIXED)
            setattr(arr[at], field, value)
            solo = C.c_char_p()
            assert lib.adc_sac_config_check(C.byref(arr[at]), C.byref(solo)) == bad
            rc, msg = _check(lib, arr, 3, 12, 3)
            assert rc == bad and msg == solo.value, (at, field)
    # with a shared configuration only the first is looked at
    arr = _configs(*MIXED)
    arr[1].gamma = 1.5
    arr[2].batch_size = 9
    assert _check(lib, arr, 1, 12, 3) == (0, None)
    rc, msg = _check(lib, None, 1, 12, 3)
    assert rc == bad and msg


def test_every_new_entry_point_is_exported_declared_and_bound(lib):
    with open(os.path.join(ROOT, "include", "adcraft_engine.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "adcraft_amd", "_ffi.py")) as f:
        ffi = f.read()
    for name in NEW_ENTRY_POINTS:
        assert getattr(lib, name) is not None                      # (AttributeError: the library does not export it)
        assert getattr(lib, name).argtypes is not None, f"{name} has no signature in _ffi"
        assert f'"{name}"' in ffi, name
        assert re.search(r"^int " + name + r"\(", header, re.M), f"{name} is not declared in include/adcraft_engine.h"
    assert lib.adc_abi_version() == 5                              # (symbols were added, nothing changed)


def test_python_surface():
    from adcraft_amd.baselines import sac_trainer
    from adcraft_amd.engine import ShardedStepEngine, StepEngine
    for name in ("mlp_learners_set_squash", "sac_pop_configs", "sac_pop_init", "sac_pop_set_critics", "sac_pop_sync_targets", "sac_pop_store",
                 "sac_pop_buffer", "sac_pop_buffer_load", "sac_pop_batch_indices", "sac_pop_update", "sac_pop_param_counts", "sac_pop_state",
                 "sac_pop_set_config", "sac_pop_copy"):
        assert callable(getattr(StepEngine, name)), name
    sharded = object.__new__(ShardedStepEngine)
    for name in ("sac_pop_init", "sac_pop_update", "mlp_learners_set_squash"):
        with pytest.raises(NotImplementedError, match="engine_shards=1"):
            getattr(sharded, name)
    arr, count = StepEngine.sac_pop_configs([dict(actor_lr=1e-5), dict(actor_lr=1e-3, optimiser="sgd", alpha_lr=0.0)], 8, 2, num_keywords=K)
    assert count == 2 and abs(arr[0].actor_lr - 1e-5) < 1e-12 and arr[1].alpha_lr == 0.0
    assert arr[0].target_entropy == -float(K + 1), "the default target entropy is -(K + 1)"
    arr, count = StepEngine.sac_pop_configs(dict(actor_lr=1e-5, target_entropy=-3.0), 8, 2)
    assert count == 1 and arr[0].target_entropy == -3.0
    with pytest.raises(ValueError, match="count"):
        StepEngine.sac_pop_configs([dict(), dict(), dict()], 8, 2, num_keywords=K)
    with pytest.raises(ValueError, match="equal"):
        StepEngine.sac_pop_configs([dict(batch_size=16), dict(batch_size=32)], 8, 2, num_keywords=K)
    with pytest.raises(ValueError, match="members"):
        StepEngine.sac_pop_configs(dict(), 9, 2, num_keywords=K)
    for name in ("iteration", "policy", "state", "copy", "set_config"):
        assert callable(getattr(sac_trainer.SACPopulationTrainer, name)), name
