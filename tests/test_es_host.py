"""The evolution strategy on the host: the twins adc_es_noise_host / adc_es_update_host (the code the device kernels run,
adc_es.h) against the numpy restatement in tests/es_ref.py bit for bit, the law optimising a quadratic, the configuration
checks and the flat parameter order.  No device is needed."""
import ctypes as C

import numpy as np
import pytest

from tests import es_ref as E
from tests import mlp_ref as R

F = np.float32


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_noise_twin_equals_the_restatement_bit_for_bit(lib):
    rng = np.random.default_rng(1)
    for seed in (1, 0xDEADBEEFCAFEF00D, 2 ** 64 - 1):
        for generation, pair in ((0, 0), (1, 0), (0, 1), (7, 31), (2 ** 31 - 1, 65535)):
            for p0, n in ((0, 64), (1, 6), (3, 1), (5, 18), (250, 9)):
                got = E.twin_noise(lib, seed, pair, generation, p0, n)
                assert _same(got, E.noise(seed, pair, generation, p0 + n, p0)), (seed, generation, pair, p0, n)
    # an unaligned range is a slice of the aligned one; pairs and generations give different draws
    full = E.twin_noise(lib, 5, 2, 3, 0, 101)
    assert _same(E.twin_noise(lib, 5, 2, 3, 17, 50), full[17:67])
    assert not np.array_equal(full, E.twin_noise(lib, 5, 3, 3, 0, 101)) and not np.array_equal(full, E.twin_noise(lib, 5, 2, 4, 0, 101))
    assert abs(float(E.twin_noise(lib, 9, 0, 0, 0, 40000).mean())) < 0.02 and abs(float(E.twin_noise(lib, 9, 0, 0, 0, 40000).std()) - 1.0) < 0.02
    del rng


def test_stage_15_is_not_the_agents_stage_14():
    """the same key draws other words on the strategy's stage than on the agents'"""
    from oracle import capi as orc
    L = orc.lib()
    key = E.es_key(77)
    a = R.normals([key], [0], 64)[0]                      # stage 14, keyword word 0, tick 0
    words = [orc.philox([q, E.ST_ES, 0, 0], [key & 0xFFFFFFFF, key >> 32]) for q in range(16)]
    b = np.array([L.orc_normal_from_word(int(w[h])) for w in words for h in range(4)], dtype=F)
    assert _same(b, E.noise(77, 0, 0, 64))
    assert not np.any(a == b)


CASES = [dict(), dict(shaping="raw"), dict(optimiser="sgd", lr=0.05), dict(l2=0.005), dict(shaping="raw", optimiser="sgd", l2=0.01, lr=0.002),
         dict(sigma=0.1, lr=0.03, beta1=0.8, beta2=0.99, eps=1e-6)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_update_twin_equals_the_restatement_bit_for_bit(lib, case):
    kw = CASES[case]
    rng = np.random.default_rng(10 + case)
    for P, M in ((64, 64), (37, 6), (5, 2)):
        theta = rng.standard_normal(P).astype(F)
        m, v = np.zeros(P, F), np.zeros(P, F)
        tw = (theta.copy(), m.copy(), v.copy())
        ref = (theta.copy(), m.copy(), v.copy())
        for generation in range(3):
            fit = rng.standard_normal(M) * 100
            if generation == 1:                               # ties, and NaNs (ranked lowest, by index)
                fit[1] = fit[0]
                fit[M - 1] = fit[0]
                if kw.get("shaping", "centered_rank") == "centered_rank":
                    fit[M // 2] = np.nan
                    fit[0 if M == 2 else 2] = np.nan
            t = E.twin_update(lib, *tw, fit, 1234 + case, generation, **kw)
            r = E.update(*ref, fit, 1234 + case, generation, **kw)
            for name, a, b in zip(("theta", "m", "v", "g"), t, r):
                assert _same(a, b), (kw, P, M, generation, name, a, b)
            assert not _same(t[0], tw[0])
            tw, ref = t[:3], r[:3]


def test_noise_twin_in_the_last_quads_of_a_wide_flat_vector(lib):
    """P = 127 345 (K = 40, hidden (256, 255, 33): tests/test_gpu_es_shapes.py holds the device to the twin there): the last 65
    parameters from an aligned start, the last 4 from p0 = 127 341 = 4 * 31 835 + 1 - quad indices above 2^14, an unaligned start,
    a last quad of one parameter"""
    P = 127345
    for seed, pair, generation in ((61, 16, 300), (2 ** 64 - 1, 0, 0), (99, 255, 301)):
        for p0 in (127280, 127341):
            got = E.twin_noise(lib, seed, pair, generation, p0, P - p0)
            assert got.size == P - p0 and _same(got, E.noise(seed, pair, generation, P, p0)), (seed, pair, generation, p0)
    assert _same(E.twin_noise(lib, 61, 16, 300, 127280, 65)[61:], E.twin_noise(lib, 61, 16, 300, 127341, 4))


@pytest.mark.parametrize("M", [34, 66])
@pytest.mark.parametrize("kw", [dict(), dict(shaping="raw", optimiser="sgd", l2=0.01, lr=0.002)], ids=["adam-ranks", "sgd-raw-l2"])
def test_update_twin_at_the_pair_counts_the_device_sums_in_rounds(lib, kw, M):
    """(P, M) = (523, 34) and (523, 66): 17 and 33 pairs, P = 4 * 130 + 3.  The twin is a serial loop and has no rounds; it is the
    yardstick of the device's rounds in tests/test_gpu_es_shapes.py, and is held to the restatement here at those counts"""
    P = 523
    rng = np.random.default_rng(200 + M)
    tw = ref = (rng.standard_normal(P).astype(F), np.zeros(P, F), np.zeros(P, F))
    for generation in range(2):
        ranks = kw.get("shaping", "centered_rank") == "centered_rank"
        fit = E.draw_fitness(rng, M, ties=generation == 1, nans=ranks and generation == 1, tie_in_pair=ranks)
        rows = E.noise_rows(77, generation, M // 2, P)
        t = E.twin_update(lib, *tw, fit, 77, generation, **kw)
        r = E.update(*ref, fit, 77, generation, rows=rows, **kw)
        for name, a, b in zip(("theta", "m", "v", "g"), t, r):
            assert _same(a, b), (kw, M, generation, name)
        # a range restated on its own is that range of the whole
        part = E.update(*(a[130:201] for a in ref), fit, 77, generation, p0=130, **kw)
        assert all(_same(a, b[130:201]) for a, b in zip(part, r)), (kw, M, generation)
        assert np.all(r[3] != 0) and not _same(t[0], tw[0])
        tw, ref = t[:3], r[:3]


def test_shaping_ranks_ties_by_index_and_nan_lowest():
    u = E.shape(np.array([3.0, np.nan, 3.0, -1.0, np.nan, 9.0]), "centered_rank")
    assert np.array_equal(u, np.array([3, 0, 4, 2, 1, 5]) / 5.0 - 0.5)


@pytest.mark.parametrize("seed", range(3))
def test_the_law_optimises_a_quadratic(lib, seed):
    """the host twin alone: P = M = 64, sigma 0.02, Adam lr 0.03, centred ranks, fitness -|theta - target|^2"""
    rng = np.random.default_rng(100 + seed)
    P = M = 64
    target = rng.standard_normal(P).astype(F)
    theta, m, v = np.zeros(P, F), np.zeros(P, F), np.zeros(P, F)
    d0 = float(np.linalg.norm(theta - target))
    for generation in range(200):
        mem = np.zeros((M, P), F)
        for i in range(M // 2):
            e = E.twin_noise(lib, seed + 1, i, generation, 0, P)
            mem[2 * i], mem[2 * i + 1] = theta + F(0.02) * e, theta + F(0.02) * (-e)
        fit = -np.sum((mem.astype(np.float64) - target) ** 2, axis=1)
        theta, m, v, _ = E.twin_update(lib, theta, m, v, fit, seed + 1, generation, sigma=0.02, lr=0.03)
    ratio = float(np.linalg.norm(theta - target)) / d0
    print("ratio", ratio)
    assert ratio < 0.1, ratio


def test_config_check(lib):
    from adcraft_amd import _ffi
    from adcraft_amd.engine import StepEngine
    ok = StepEngine.es_config()
    assert ok.struct_size == C.sizeof(_ffi.ESConfig) and abs(ok.sigma - 0.02) < 1e-9 and abs(ok.lr - 0.01) < 1e-9
    for bad in (dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(lr=-0.1), dict(beta1=1.0),
                dict(beta2=-0.1), dict(eps=0.0), dict(l2=-1.0)):
        with pytest.raises(ValueError):
            StepEngine.es_config(**bad)
    StepEngine.es_config(optimiser="sgd", beta1=1.0, eps=0.0)      # (Adam's constants are not SGD's business)
    msg = C.c_char_p()
    c = StepEngine.es_config()
    c.struct_size = 4
    assert lib.adc_es_config_check(C.byref(c), C.byref(msg)) == _ffi.ADC_EINVAL and b"struct_size" in msg.value
    assert lib.adc_es_config_check(None, None) == _ffi.ADC_EINVAL
    c = StepEngine.es_config()
    c.shaping = 9
    assert lib.adc_es_config_check(C.byref(c), None) == _ffi.ADC_EINVAL
    # the twin refuses what the engine would: odd members, no members
    th = np.zeros(4, F)
    fit = np.zeros(3)
    c = StepEngine.es_config()
    assert lib.adc_es_update_host(C.byref(c), 1, 3, 4, fit.ctypes.data, 0, th.ctypes.data, th.ctypes.data, th.ctypes.data, None) == _ffi.ADC_EINVAL


def test_flat_parameter_order_round_trips_through_the_policy():
    from adcraft_amd.baselines.es_trainer import flat_params, policy_from_flat
    rng = np.random.default_rng(4)
    K = 7
    pol = R.random_policy(rng, K, (16, 8), "tanh", value=True)
    flat = flat_params(pol)
    D, A = 5 * K + 2, K + 1
    assert flat.size == D * 16 + 16 + 16 * 8 + 8 + 8 * A + A and flat.dtype == F
    w0, b0 = pol.layers[0]
    assert flat[3 * 16 + 5] == w0[3, 5] and _same(flat[D * 16:D * 16 + 16], b0)
    assert _same(flat, E.flat_params(pol))
    back = policy_from_flat(pol, flat)
    for (w, b), (w2, b2) in zip(pol.layers, back.layers):
        assert _same(w, w2) and _same(b, b2)
    assert back.value_layers is pol.value_layers or all(_same(a[0], b[0]) for a, b in zip(back.value_layers, pol.value_layers))
    other = policy_from_flat(pol, flat + F(1))
    assert _same(flat_params(other), flat + F(1)) and _same(flat_params(pol), flat)          # (the original is untouched)
    with pytest.raises(ValueError):
        policy_from_flat(pol, flat[:-1])
