"""Prioritised replay on the host: the twins adc_per_tree_host / adc_per_descend_host / adc_per_sample_host / adc_per_priority_host /
adc_per_leaf_update_host (the code the device kernels run, adc_per.h) against the numpy restatement in tests/per_ref.py bit for bit -
the tree for one, two (padded) and three levels and for size < C, the descent and its "no child found" fall-back, the weights, the
priority clamp with a NaN, the max over duplicates - one distribution check of the sampler, the configuration checks and the Python
surface.  No device is needed.  None of these symbols exists before this feature."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import per_ref as PR

F = np.float32
D64 = np.float64


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _leaves(rng, size):
    """positive leaves spread over three decades"""
    return (10.0 ** rng.uniform(-2, 1, size)).astype(F)


# capacity, stored slots: one level; a padded second level; three levels; size < C for each
SHAPES = [(64, 64), (64, 9), (100, 100), (100, 65), (4100, 4100), (4100, 4097), (4100, 130), (1, 1), (4096, 4096)]


@pytest.mark.parametrize("capacity,size", SHAPES)
def test_tree_equals_the_restatement(lib, capacity, size):
    rng = np.random.default_rng(capacity * 7 + size)
    leaf = _leaves(rng, size)
    ref = PR.Tree(capacity, leaf)
    L, counts, nodes = PR.twin_tree(lib, capacity, leaf)
    assert L == ref.L and list(counts) == ref.n
    assert L == max(1, math.ceil(math.log(capacity, 64) - 1e-12))
    assert _same(nodes, ref.nodes())
    # a node is its children's plain sum up to the scan's rounding, and the root the leaves'
    assert abs(ref.total - leaf.astype(D64).sum()) <= 1e-12 * ref.total


@pytest.mark.parametrize("capacity,size", SHAPES)
def test_descent_and_weights_equal_the_restatement(lib, capacity, size):
    rng = np.random.default_rng(capacity * 11 + size)
    leaf = _leaves(rng, size)
    ref = PR.Tree(capacity, leaf)
    for m in np.concatenate([[0.0], rng.random(24) * ref.total]):
        slot = PR.twin_descend(lib, capacity, leaf, m)
        assert slot == ref.descend(m) and 0 <= slot < size
        # the slot is the one whose interval of the running sum holds m (up to the scans' rounding at an edge)
        cum = np.cumsum(leaf.astype(D64))
        assert cum[slot] >= m * (1 - 1e-12) and (slot == 0 or cum[slot - 1] <= m * (1 + 1e-12))
    for update, beta in ((0, 0.4), (3, 1.0), (2 ** 32 - 2, 0.0)):
        B = 33
        idx, w = PR.twin_sample(lib, capacity, size, leaf, 1234, update, B, beta=beta)
        ridx, rw = PR.sample(ref, 1234, update, B, size, beta)
        assert _same(idx, ridx) and _same(w, rw)
        assert idx.min() >= 0 and idx.max() < size and w.max() == 1 and w.min() > 0
        if beta == 0.0:
            assert np.all(w == 1)


def test_no_child_found_falls_back_to_the_last_nonzero_child(lib):
    """m = total: no prefix exceeds it at the root; the descent takes the last child with a nonzero value, there and below"""
    for capacity, size in ((64, 40), (100, 70), (4100, 4000)):
        leaf = _leaves(np.random.default_rng(capacity), size)
        ref = PR.Tree(capacity, leaf)
        for m in (ref.total, ref.total * 2):
            slot = PR.twin_descend(lib, capacity, leaf, m)
            assert slot == ref.descend(m) == size - 1
    # an empty tree: child 0 all the way down
    assert PR.twin_descend(lib, 100, np.zeros(0, F), 0.0) == PR.Tree(100).descend(0.0) == 0


def test_priority_clamp(lib):
    nan, inf = F(np.nan), F(np.inf)
    d1 = np.array([0, 1e-9, 0.5, -3, 1e7, nan, inf, -inf, 2, 1e-3], F)
    d2 = np.array([0, 0, -0.25, 5, 1e7, 1, 1, nan, -2, -1e-3], F)
    for per in (dict(alpha=0.6, eps=1e-6, cap=1e6), dict(alpha=1.0, eps=1e-2, cap=4.0), dict(alpha=0.0, eps=1e-6, cap=1e6)):
        p = PR.priority(d1, d2, per["eps"], per["cap"])
        assert p[0] == F(per["eps"]) and p[5] == F(per["eps"]) and p[7] == F(per["eps"]) and p[4] == F(per["cap"]) and p[6] == F(per["cap"])
        assert np.all(p >= F(per["eps"])) and np.all(p <= F(per["cap"]))
        out = PR.twin_priority(lib, d1, d2, **per)
        assert _same(out, PR.pa(p, per["alpha"]))
        if per["alpha"] == 0.0:
            assert np.all(out == 1)
        if per["alpha"] == 1.0:
            np.testing.assert_allclose(out, p, rtol=1e-6)


def test_leaf_update_takes_the_maximum_over_duplicates(lib):
    rng = np.random.default_rng(5)
    capacity, size, B = 100, 8, 16
    leaf = _leaves(rng, size)
    idx = rng.integers(0, size, B).astype(np.int32)
    idx[:4] = 3                                         # a slot drawn four times
    pab = _leaves(rng, B)
    ref = PR.Tree(capacity, leaf, top=0.5)
    PR.leaf_update(ref, idx, pab)
    lf, top = PR.twin_leaf_update(lib, capacity, leaf, 0.5, idx, pab)
    assert _same(lf, ref.leaf[:capacity]) and top == ref.top == max(F(0.5), pab.max())
    assert lf[3] == pab[idx == 3].max()
    untouched = np.setdiff1d(np.arange(size), idx)
    assert _same(lf[untouched], leaf[untouched])
    # the paths were rebuilt: the restatement's nodes are the twin's tree over the new leaves
    assert _same(PR.twin_tree(lib, capacity, lf)[2], ref.nodes())
    # a lower batch leaves top alone
    assert PR.twin_leaf_update(lib, capacity, leaf, 100.0, idx, pab)[1] == F(100.0)


def _chi2_quantile(p, k):
    """the p-quantile of chi-square with k degrees of freedom: bisection on the regularised lower incomplete gamma P(k / 2, x / 2),
    from its series (x < a + 1) or Lentz's continued fraction for Q"""
    a = k / 2.0

    def cdf(x):
        x = x / 2.0
        if x < a + 1:
            term = total = 1.0 / a
            n = a
            while abs(term) > 1e-17 * abs(total):
                n += 1
                term *= x / n
                total += term
            return total * math.exp(-x + a * math.log(x) - math.lgamma(a))
        b, c, d = x + 1 - a, 1e300, 1.0 / (x + 1 - a)
        h = d
        for i in range(1, 2000):
            an = -i * (i - a)
            b += 2
            d = 1.0 / (an * d + b)
            c = b + an / c
            h *= d * c
            if abs(d * c - 1) < 1e-16:
                break
        return 1.0 - h * math.exp(-x + a * math.log(x) - math.lgamma(a))

    lo, hi = 0.0, 10.0 * k
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if cdf(mid) < p else (lo, mid)
    return 0.5 * (lo + hi)


def test_the_sampler_draws_in_proportion_to_the_leaves(lib):
    """64 slots with leaves spread over three decades, 4096 draws of the host twin under a fixed seed: Pearson's statistic against
    leaf / total is below the 0.999 quantile of chi-square with 63 degrees of freedom, 103.4424"""
    q = _chi2_quantile(0.999, 63)
    assert abs(q - 103.4424) < 1e-3
    leaf = (10.0 ** np.linspace(-1.5, 1.5, 64)).astype(F)
    idx, _ = PR.twin_sample(lib, 64, 64, leaf, 2024, 0, 4096, beta=0.4)
    counts = np.bincount(idx, minlength=64).astype(D64)
    expect = 4096 * leaf.astype(D64) / leaf.astype(D64).sum()
    stat = float(((counts - expect) ** 2 / expect).sum())
    print(f"Pearson statistic {stat:.3f}, bound {q:.4f}")
    assert stat < q


def test_config_check(lib):
    from adcraft_amd import _ffi
    from adcraft_amd.engine import StepEngine
    good = StepEngine.replay_prio_config()
    assert (good.alpha, good.beta, good.eps, good.cap) == (F(0.6), F(0.4), F(1e-6), F(1e6))
    StepEngine.replay_prio_config(alpha=0, beta=0)
    StepEngine.replay_prio_config(alpha=1, beta=1, eps=1e-3, cap=2e-3)
    for bad in (dict(alpha=-0.1), dict(alpha=1.1), dict(alpha=float("nan")), dict(beta=-0.1), dict(beta=1.5), dict(beta=float("nan")), dict(eps=0.0),
                dict(eps=-1.0), dict(eps=float("inf")), dict(eps=float("nan")), dict(cap=1e-6), dict(cap=1e-7), dict(cap=float("inf")),
                dict(cap=float("nan"))):
        with pytest.raises(ValueError):
            StepEngine.replay_prio_config(**bad)
    msg = C.c_char_p()
    assert lib.adc_replay_prio_config_check(None, C.byref(msg)) == _ffi.ADC_EINVAL and msg.value
    good.struct_size -= 4
    assert lib.adc_replay_prio_config_check(C.byref(good), None) == _ffi.ADC_EINVAL
    # the twins refuse what the law has no answer for
    leaf = np.ones(4, F)
    cfg = StepEngine.replay_prio_config()
    idx = np.zeros(2, np.int32)
    assert lib.adc_per_sample_host(C.byref(cfg), 4, 5, leaf.ctypes.data, 1, 0, 2, idx.ctypes.data, None) == _ffi.ADC_EINVAL      # size > capacity
    assert lib.adc_per_sample_host(C.byref(cfg), 4, 0, leaf.ctypes.data, 1, 0, 2, idx.ctypes.data, None) == _ffi.ADC_EINVAL      # an empty ring
    assert lib.adc_per_tree_host(0, leaf.ctypes.data, None, None) == _ffi.ADC_EINVAL
    bad = np.array([1, -1, 1, 1], F)
    assert lib.adc_per_tree_host(4, bad.ctypes.data, None, None) == _ffi.ADC_EINVAL
