"""N-step returns on the host: the twins adc_replay_nstep_host / adc_td3_y_nstep_host / adc_sac_y_nstep_host (the code the device
kernels run, adc_td3.h "n-step") against the numpy restatement in tests/nstep_ref.py bit for bit - windows cut by done flags on
the first, the last and two consecutive days and by the fragment's end, t0 > 0, -0.0 rewards, gamma 0.995, 1 and 0 - hand-written
windows, n = 1, the targets with gn = gamma against the existing twins, the refusals and the trainers' shared n_step.  No device
is needed.  None of these symbols exists before this feature."""
import ctypes as C

import numpy as np
import pytest

from tests import nstep_ref as NS
from tests import sac_norm_ref as SN
from tests import td3_norm_ref as TN

F = np.float32


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _record(rng, T, N, where):
    """rewards with a -0.0 among them; done flags (terminated or truncated, never needed both) by `where`"""
    reward = (rng.standard_normal((T, N)) * 3).astype(F)
    reward[rng.integers(0, T), rng.integers(0, N)] = F(-0.0)
    term, trunc = np.zeros((T, N), bool), np.zeros((T, N), bool)
    if where == "first":
        term[0, :] = True
    elif where == "last":
        trunc[T - 1, :] = True
    elif where == "consecutive":
        term[min(1, T - 1), 0] = True
        trunc[min(2, T - 1), 0] = True
        term[0, 1] = trunc[min(1, T - 1), 1] = True
        term[T // 2, 2] = trunc[T // 2, 2] = True           # both flags on one day
    return reward, term, trunc


def _assert_windows(got, ref, what):
    for k in ("m", "R", "done", "gn"):
        assert _same(got[k], ref[k]), (k, what, got[k], ref[k])


@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 16])
def test_twin_equals_the_restatement(lib, T, n):
    N = 3
    rng = np.random.default_rng(100 * T + n)
    for where in ("first", "last", "consecutive", "nowhere"):
        reward, term, trunc = _record(rng, T, N, where)
        for gamma in (0.995, 1.0, 0.0):
            for t0 in sorted({0, T - 1, T // 2}):
                ref = NS.windows(n, gamma, reward, term, trunc, t0)
                got = NS.twin_windows(lib, n, gamma, reward, term, trunc, t0)
                _assert_windows(got, ref, (where, gamma, t0))
                assert ref["m"].min() >= 1 and ref["m"].max() <= min(n, T - t0)
                # the fragment's end cuts the window: a sample of the last day has m = 1 and its own reward and flag
                last = slice((T - 1 - t0) * N, (T - t0) * N)
                assert np.all(ref["m"][last] == 1) and _same(ref["R"][last], reward[T - 1]) and _same(ref["done"][last], (term | trunc)[T - 1])
                assert np.all(ref["gn"][last] == F(gamma))
    # a fragment that ends before the record does: the days past t1 are not read
    if T == 5:
        reward, term, trunc = _record(rng, T, N, "nowhere")
        ref = NS.windows(n, 0.995, reward, term, trunc, 1, 4)
        _assert_windows(NS.twin_windows(lib, n, 0.995, reward, term, trunc, 1, 4), ref, "t1 < T")
        poisoned = reward.copy()
        poisoned[4] = np.nan
        _assert_windows(NS.twin_windows(lib, n, 0.995, poisoned, term, trunc, 1, 4), ref, "t1 < T, day 4 poisoned")


def test_n_1_is_the_one_step_transition(lib):
    rng = np.random.default_rng(7)
    for where in ("first", "last", "consecutive", "nowhere"):
        reward, term, trunc = _record(rng, 5, 3, where)
        for gamma in (0.995, 1.0, 0.0):
            got = NS.twin_windows(lib, 1, gamma, reward, term, trunc, 1)
            assert _same(got["R"], reward[1:].reshape(-1)) and _same(got["done"], (term | trunc)[1:].reshape(-1))
            assert _same(got["gn"], np.full(12, gamma, F)) and np.all(got["m"] == 1)


def test_hand_written_windows(lib):
    z = np.zeros((4, 1), bool)
    r = np.array([[1], [2], [4], [8]], F)
    # gamma 0.5, n 3: 1 + 0.5 * 2 + 0.25 * 4 = 3 with gn 0.125; 2 + 2 + 2 = 6; the fragment's end: 4 + 4 = 8 (m 2), 8 (m 1)
    for w in (NS.windows(3, 0.5, r, z, z), NS.twin_windows(lib, 3, 0.5, r, z, z)):
        assert w["R"].tolist() == [3.0, 6.0, 8.0, 8.0] and w["gn"].tolist() == [0.125, 0.125, 0.25, 0.5]
        assert w["m"].tolist() == [3, 3, 2, 1] and w["done"].tolist() == [False] * 4
    # day 1 ends an episode: day 0's window stops there and carries its flag; day 1 is alone; day 2 starts anew
    term = np.array([[0], [1], [0], [0]], bool)
    for w in (NS.windows(3, 0.5, r, term, z), NS.twin_windows(lib, 3, 0.5, r, term, z)):
        assert w["R"].tolist() == [2.0, 2.0, 8.0, 8.0] and w["gn"].tolist() == [0.25, 0.5, 0.25, 0.5]
        assert w["m"].tolist() == [2, 1, 2, 1] and w["done"].tolist() == [True, True, False, False]
    # truncated counts as terminated; n larger than the record; gamma 1 sums plainly and leaves gn = 1
    trunc = np.array([[0], [0], [1], [0]], bool)
    for w in (NS.windows(16, 1.0, r, z, trunc), NS.twin_windows(lib, 16, 1.0, r, z, trunc)):
        assert w["R"].tolist() == [7.0, 6.0, 4.0, 8.0] and w["gn"].tolist() == [1.0] * 4
        assert w["m"].tolist() == [3, 2, 1, 1] and w["done"].tolist() == [True, True, True, False]
    # gamma 0: the later rewards enter as +-0 products, gn is 0 from the second day on
    for w in (NS.windows(3, 0.0, r, z, z), NS.twin_windows(lib, 3, 0.0, r, z, z)):
        assert w["R"].tolist() == [1.0, 2.0, 4.0, 8.0] and w["gn"].tolist() == [0.0, 0.0, 0.0, 0.0] and w["m"].tolist() == [3, 3, 2, 1]
    # gn is gamma multiplied m - 1 times by gamma in float32, not a power taken elsewhere
    g = F(0.995)
    w = NS.twin_windows(lib, 16, g, np.ones((16, 1), F), np.zeros((16, 1), bool), np.zeros((16, 1), bool))
    acc = g
    for _ in range(15):
        acc = F(acc * g)
    assert w["m"][0] == 16 and w["gn"][0] == acc
    # two envs: a window walks its own env's column
    r2 = np.array([[1, 10], [2, 20], [4, 40]], F)
    t2 = np.array([[0, 1], [0, 0], [0, 0]], bool)
    w = NS.twin_windows(lib, 2, 0.5, r2, t2, np.zeros((3, 2), bool))
    assert w["R"].tolist() == [2.0, 10.0, 4.0, 40.0, 4.0, 40.0] and w["m"].tolist() == [2, 1, 2, 2, 1, 1]


def test_target_twins(lib):
    rng = np.random.default_rng(11)
    B, gamma, rsc, alpha = 37, 0.97, 0.5, 0.3
    r, q, lp = (rng.standard_normal(B) * 4).astype(F), (rng.standard_normal(B) * 2).astype(F), (rng.standard_normal(B) * 3).astype(F)
    done = rng.random(B) < 0.3
    const = np.full(B, gamma, F)
    for scale, clip in ((1.0, 0.0), (0.37, 0.0), (0.37, 1.25)):
        # gn = gamma: the existing twins' bits
        assert _same(NS.twin_td3_y(lib, r, done, q, const, gamma, rsc, scale, clip), TN.twin_y(lib, r, done, q, gamma, rsc, scale, clip))
        assert _same(NS.twin_sac_y(lib, r, done, q, alpha, lp, const, gamma, rsc, scale, clip), SN.twin_y(lib, r, done, q, alpha, lp, gamma, rsc, scale, clip))
        # a discount per element, gamma to gamma^3 and a free one: the restatement's bits
        gn = np.where(rng.random(B) < 0.5, F(gamma), F(F(gamma) * F(gamma)))
        gn[::5] = F(F(F(gamma) * F(gamma)) * F(gamma))
        gn[1::7] = rng.random(len(gn[1::7])).astype(F)
        assert _same(NS.twin_td3_y(lib, r, done, q, gn, gamma, rsc, scale, clip), NS.td3_y(r, done, q, gn, rsc, scale, clip))
        assert _same(NS.twin_sac_y(lib, r, done, q, alpha, lp, gn, gamma, rsc, scale, clip), NS.sac_y(r, done, q, alpha, lp, gn, rsc, scale, clip))
    # without the multiplier and the clip: td3_y / sac_y themselves
    assert _same(NS.twin_td3_y(lib, r, done, q, gn, gamma, rsc), NS.td3_y(r, done, q, gn, rsc))
    assert _same(NS.twin_sac_y(lib, r, done, q, alpha, lp, gn, gamma, rsc), NS.sac_y(r, done, q, alpha, lp, gn, rsc))
    assert _same(NS.td3_y(r, done, q, const, rsc), TN.y_plain(r, done, q, gamma, rsc))
    assert _same(NS.sac_y(r, done, q, alpha, lp, const, rsc), SN.y_plain(r, done, q, alpha, lp, gamma, rsc))
    assert not _same(NS.td3_y(r, done, q, gn, rsc), TN.y_plain(r, done, q, gamma, rsc))


def test_refusals(lib):
    from adcraft_amd import _ffi
    msg = C.c_char_p()
    for n in range(1, 17):
        assert lib.adc_replay_nstep_check(n, C.byref(msg)) == _ffi.ADC_OK and msg.value is None
    r, z = np.ones((2, 1), F), np.zeros((2, 1), bool)
    for n in (0, -1, 17, 2 ** 31 - 1, -2 ** 31):
        msg = C.c_char_p()
        assert lib.adc_replay_nstep_check(n, C.byref(msg)) == _ffi.ADC_EINVAL and msg.value, n
        assert lib.adc_replay_nstep_check(n, None) == _ffi.ADC_EINVAL
        assert NS.twin_windows(lib, n, 0.9, r, z, z) == _ffi.ADC_EINVAL
    # a fragment outside the record, or an empty one
    assert NS.twin_windows(lib, 2, 0.9, r, z, z, 0, 3) == _ffi.ADC_EINVAL
    assert NS.twin_windows(lib, 2, 0.9, r, z, z, 1, 1) == _ffi.ADC_EINVAL
    assert NS.twin_windows(lib, 2, 0.9, r, z, z, -1, 1) == _ffi.ADC_EINVAL
    assert lib.adc_replay_nstep_host(2, 0.9, 2, 1, 0, 2, None, None, None, None, None, None, None) == _ffi.ADC_EINVAL


def test_trainers_refuse_a_bad_or_a_differing_n_step():
    from adcraft_amd.baselines.sac_trainer import SACPopulationTrainer, SACTrainer
    from adcraft_amd.baselines.td3_trainer import TD3PopulationTrainer, TD3Trainer, nstep_check
    assert [nstep_check(n) for n in (1, 3, 16)] == [1, 3, 16]
    for bad in (0, 17, -3, 2.5, True):
        with pytest.raises(ValueError, match="n_step"):
            nstep_check(bad)
        # (refused before the engine or the policy is touched)
        with pytest.raises(ValueError, match="n_step"):
            TD3Trainer(None, object(), n_step=bad)
        with pytest.raises(ValueError, match="n_step"):
            SACTrainer(None, object(), 0.0, 1.0, n_step=bad)
    with pytest.raises(ValueError, match="n_step is shared"):
        TD3PopulationTrainer(None, object(), None, [dict(n_step=3), dict(n_step=2)])
    with pytest.raises(ValueError, match="n_step is shared"):
        TD3PopulationTrainer(None, object(), None, [dict(n_step=3), dict()])
    with pytest.raises(ValueError, match="n_step is shared"):
        SACPopulationTrainer(None, object(), [dict(n_step=1), dict(n_step=2)], 0.0, 1.0)
    with pytest.raises(ValueError, match="n_step"):
        SACPopulationTrainer(None, object(), dict(n_step=17), 0.0, 1.0)
