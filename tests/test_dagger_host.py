"""DAgger on the host: the exported symbols, the coin's twin adc_dagger_coin_host (the code k_dagger_mix runs, adc_dagger.h)
against the numpy restatement in tests/dagger_ref.py, the two ends of beta, and that the inputs of the mixed GPU test
(tests/test_gpu_dagger.py) exercise both branches.  No device is needed."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import dagger_ref as DR
from tests import mlp_ref as R

F = np.float32
NEW_SYMBOLS = ("adc_engine_dagger_days", "adc_engine_dagger_mask_fetch", "adc_dagger_coin_host")
BELOW_ONE = float(np.nextafter(F(1), F(0)))
BETAS = (0.0, 2.0 ** -32, 0.5, BELOW_ONE, 1.0)
# the mixed GPU test's inputs: agent seeds arange(6) + 11, the ticks of its four days, beta 0.5
MIX_SEEDS, MIX_DAYS, MIX_BETA = np.arange(6, dtype=np.uint64) + 11, 4, 0.5


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def test_the_new_symbols_are_exported_and_the_abi_is_unchanged(lib):
    from adcraft_amd import _ffi
    header = (Path(__file__).resolve().parents[1] / "include" / "adcraft_engine.h").read_text()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
        assert re.search(rf"\bint {name}\(", header), name
    assert lib.adc_abi_version() == 5 and lib.adc_stream_revision() == 5
    assert (_ffi.ABI_VERSION, _ffi.STREAM_REVISION) == (5, 5)


def test_the_threshold_is_the_laws(lib):
    assert [DR.threshold(b) for b in BETAS] == [0, 1, 1 << 31, (1 << 32) - 256, 1 << 32]
    assert DR.threshold(float("nan")) == 0 and DR.threshold(-0.5) == 0 and DR.threshold(2.0) == 1 << 32
    from oracle import capi as orc
    rng = np.random.default_rng(2)
    for b in list(BETAS) + list(rng.random(200).astype(F)) + list((rng.random(50) * 1e-6).astype(F)):
        assert DR.threshold(b) == int(orc.lib().orc_bernoulli_threshold(float(F(b)))), b


def test_the_coin_twin_equals_the_restatement(lib):
    rng = np.random.default_rng(31)
    keys = [R.agent_key(s) for s in range(11, 17)] + [int(k) for k in rng.integers(0, 2 ** 63, 10)] + [0, 2 ** 64 - 1]
    ticks = [0, 1, 2, 3, 7, 255, 65536, 2 ** 31, 2 ** 32 - 1]
    seen = set()
    for beta in BETAS:
        for tick in ticks:
            want = DR.coin(keys, [tick] * len(keys), beta)
            got = np.array([lib.adc_dagger_coin_host(k, tick, beta) for k in keys], np.uint8)
            assert np.array_equal(got, want), (beta, tick)
            seen.update((beta, int(c)) for c in want)
    assert (0.5, 0) in seen and (0.5, 1) in seen
    # the coin is word x of the stage-23 call and nothing else: the smallest nonzero beta picks the teacher exactly when it is 0
    assert all(DR.coin([k], [t], 2.0 ** -32)[0] == (DR.word(k, t) == 0) for k in keys for t in ticks)


def test_beta_zero_never_and_beta_one_always_picks_the_teacher(lib):
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 2 ** 63, 3000)
    ticks = rng.integers(0, 2 ** 32, 3000)
    ones = zeros = below = 0
    for k, t in zip(keys, ticks):
        zeros += lib.adc_dagger_coin_host(int(k), int(t), 0.0)
        ones += lib.adc_dagger_coin_host(int(k), int(t), 1.0)
        below += lib.adc_dagger_coin_host(int(k), int(t), 0.5)
    assert zeros == 0 and ones == 3000
    assert 1350 < below < 1650, "a fair coin over 3000 draws: six standard deviations are 164"


def test_the_mixed_gpu_tests_inputs_exercise_both_branches():
    keys = [R.agent_key(s) for s in MIX_SEEDS]
    mask = DR.mask(keys, np.zeros(len(keys), np.int64), MIX_DAYS, MIX_BETA)
    assert mask.shape == (MIX_DAYS, len(keys))
    assert mask[0].tolist() == [0, 1, 1, 1, 0, 1]
    assert (mask.min(axis=0) == 0).all() and (mask.max(axis=0) == 1).all(), "every env has both values within the four days"
