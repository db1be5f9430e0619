"""The PPO learners' shuffled sample-level minibatches on the host: the twins adc_pg_shuffle_order_host / adc_pg_shuffle_stop_host
(the code the device kernels run, adc_pg_shuffle.h) against the numpy restatement in tests/pg_shuffle_ref.py, that the order is a
permutation and behaves as a shuffle, the configuration check and the Python surface.  No device is needed."""
import ctypes as C

import numpy as np
import pytest

from tests import pg_shuffle_ref as S

F = np.float32
SIZES = (1, 2, 3, 4, 5, 16, 17, 40, 1024, 1025, 2064)


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


# ---- 1. the order ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s", SIZES)
def test_the_order_is_the_restatements_and_a_permutation(lib, n_s):
    """b = 2 (n_s up to 4), exact powers of four (no walk: 4, 16, 1024) and one past them (5, 17, 1025), 2064 as the device
    tests use it: the twin's order equals the restatement's and is a permutation; two ticks and two seeds give different orders
    (asserted from 16 samples on: with five or fewer, two of the few possible orders may well coincide)"""
    seen = []
    for seed, tick in ((7, 0), (7, 1), (8, 0), (7, 0xFFFFFFFF)):
        got = S.twin_order(lib, seed, n_s, tick)
        ref = S.order(seed, n_s, tick)
        assert got.dtype == ref.dtype and np.array_equal(got, ref), (seed, tick)
        assert np.array_equal(np.sort(got), np.arange(n_s, dtype=np.uint32)), (seed, tick)
        seen.append(got)
    if n_s >= 16:
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], seen[2]) and not np.array_equal(seen[0], seen[3])
    assert S.half_bits(n_s) * 2 == max(2, 2 * int(np.ceil(np.log2(max(n_s, 2)) / 2)))


def test_the_order_refuses_bad_arguments(lib):
    out = np.zeros(4, np.uint32)
    assert lib.adc_pg_shuffle_order_host(1, 0, 0, out.ctypes.data) != 0
    assert lib.adc_pg_shuffle_order_host(1, 1 << 31, 0, out.ctypes.data) != 0
    assert lib.adc_pg_shuffle_order_host(1, 4, 0, None) != 0


# ---- 2. the order behaves as a shuffle -----------------------------------------------------------------------------------------------
def test_the_order_behaves_as_a_shuffle(lib):
    """n_s = 2064 (344 envs x 6 days), ticks 0 .. 1999: the number of positions [0, 64) - one minibatch - that hold a sample of
    day 0 (index below 344) is hypergeometric under a uniform shuffle: mean 64 * 344 / 2064 = 10.667, variance 8.62, so the mean
    over 2000 draws lies within 4 standard errors = 0.26 of it; a uniform permutation has one fixed point on average (variance
    1: the mean over 2000 within 0.1 is 4.5 standard errors).  A fixed, deterministic input: if this fails the law is wrong."""
    n_s, ticks = 2064, 2000
    first, fixed = np.zeros(ticks), np.zeros(ticks)
    ident = np.arange(n_s, dtype=np.uint32)
    for k in range(ticks):
        o = S.twin_order(lib, 12345, n_s, k)
        first[k] = np.count_nonzero(o[:64] < 344)
        fixed[k] = np.count_nonzero(o == ident)
    print(f"mean count of day-0 samples in the first minibatch {first.mean():.4f} (10.667), mean fixed points {fixed.mean():.4f} (1)")
    assert abs(first.mean() - 64 * 344 / 2064) <= 0.26, first.mean()
    assert abs(fixed.mean() - 1.0) <= 0.1, fixed.mean()


# ---- 3. the configuration check and the stop rule --------------------------------------------------------------------------------------
def test_config_check_refusals(lib):
    from adcraft_amd import _ffi
    from adcraft_amd.engine import StepEngine
    good = StepEngine.pg_shuffle_config(minibatch_samples=64, seed=3, target_kl=0.01)
    assert (good.minibatch_samples, good.seed, good.struct_size) == (64, 3, C.sizeof(_ffi.PGShuffleConfig)) and good.target_kl == F(0.01)
    msg = C.c_char_p()
    assert lib.adc_pg_shuffle_config_check(C.byref(good), C.byref(msg)) == _ffi.ADC_OK and msg.value is None
    assert lib.adc_pg_shuffle_config_check(None, C.byref(msg)) == _ffi.ADC_EINVAL and b"struct_size" in msg.value
    for field, value, word in (("struct_size", 4, "struct_size"), ("minibatch_samples", 0, "minibatch_samples"), ("minibatch_samples", -3, "minibatch_samples"),
                               ("target_kl", -1e-3, "target_kl"), ("target_kl", float("nan"), "target_kl"), ("target_kl", float("inf"), "target_kl")):
        bad = StepEngine.pg_shuffle_config()
        setattr(bad, field, value)
        assert lib.adc_pg_shuffle_config_check(C.byref(bad), C.byref(msg)) == _ffi.ADC_EINVAL, (field, value)
        assert word.encode() in msg.value, (field, msg.value)
    for kw in (dict(minibatch_samples=0), dict(target_kl=-1.0), dict(target_kl=float("nan"))):
        with pytest.raises(ValueError):
            StepEngine.pg_shuffle_config(**kw)


def test_the_stop_rule_at_its_bound(lib):
    """approx_kl equal to, just below and just above 1.5 * float64(float32(target_kl)); target_kl = 0 never stops"""
    for target in (0.01, 0.3, 1e-6):
        bound = 1.5 * np.float64(F(target))
        for kl, want in ((bound, False), (np.nextafter(bound, -np.inf), False), (np.nextafter(bound, np.inf), True), (0.0, False), (-1.0, False),
                         (10.0 * bound, True), (float("nan"), False)):
            assert S.twin_stop(lib, kl, target) is want, (target, kl)
            assert S.stop(kl, target) is want, (target, kl)
    for kl in (0.0, 1.0, 1e30, float("inf")):
        assert S.twin_stop(lib, kl, 0.0) is False and S.stop(kl, 0.0) is False
    out = C.c_int32(0)
    assert lib.adc_pg_shuffle_stop_host(0.1, -1.0, C.byref(out)) != 0 and lib.adc_pg_shuffle_stop_host(0.1, 0.1, None) != 0


# ---- 4. the Python layer ----------------------------------------------------------------------------------------------------------------
RLLIB_PPO = dict(epochs=20, minibatches=4, gamma=0.995, lam=0.95, eps_clip=0.5, vf_coef=2.0, ent_coef=0.0, normalize_advantages=True, max_grad_norm=0.5,
                 optimiser="adam", lr=1e-4, kl_penalty=dict(kl_coef=1.0, kl_target=0.01, adaptive=True, vf_clip=10.0))


def test_rllib_ppo_keeps_what_it_returned_and_carries_the_size():
    from adcraft_amd.baselines import pg_trainer
    assert pg_trainer.rllib_ppo() == RLLIB_PPO
    assert pg_trainer.rllib_ppo(lr=3e-4) == dict(RLLIB_PPO, lr=3e-4)
    with64 = pg_trainer.rllib_ppo(minibatch_size=64)
    assert with64 == dict({k: v for k, v in RLLIB_PPO.items() if k != "minibatches"}, minibatch_size=64)
    assert "NOT reproduce" not in pg_trainer.rllib_ppo.__doc__ and "sgd_minibatch_size" in pg_trainer.rllib_ppo.__doc__


class _NoEngine:
    """the trainers must refuse before they touch the engine"""
    num_envs = 8

    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched ({name}) before the configuration was checked")


def test_minibatches_and_minibatch_size_exclude_each_other():
    from adcraft_amd.baselines.pg_trainer import PGPopulationTrainer, PGTrainer
    with pytest.raises(ValueError, match="minibatch_size"):
        PGTrainer(_NoEngine(), None, 4, minibatches=2, minibatch_size=16)
    with pytest.raises(ValueError, match="minibatch_size"):
        PGTrainer(_NoEngine(), None, 4, target_kl=0.01)
    with pytest.raises(ValueError, match="minibatch_size"):
        PGTrainer(_NoEngine(), None, 4, minibatch_size=0)

    class Pol:
        shift = None

        def shapes(self):
            return ()
    with pytest.raises(ValueError, match="minibatch_size"):
        PGPopulationTrainer(_NoEngine(), [Pol(), Pol()], 4, [dict(minibatch_size=16, minibatches=2), dict(minibatch_size=16)])
    with pytest.raises(ValueError, match="some members"):
        PGPopulationTrainer(_NoEngine(), [Pol(), Pol()], 4, [dict(minibatch_size=16), dict()])
    with pytest.raises(ValueError, match="equal in all"):
        PGPopulationTrainer(_NoEngine(), [Pol(), Pol()], 4, [dict(minibatch_size=16), dict(minibatch_size=8)])
