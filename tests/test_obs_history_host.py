"""The observation history on the host: the twin adc_mlp_stack_row_host (the code the device's prologue runs, adc_mlp.h) against
the numpy restatement in tests/stack_ref.py bit for bit over random sequences of acts - day 0, skipped days, a second act on the
same day, peeks, explicit-reset forgets - and MLPPolicy(frames=...)'s validation and refusals.  No device is needed.  None of
these symbols exists before this feature."""
import numpy as np
import pytest

from tests import mlp_ref as R
from tests import stack_ref as S

F = np.float32


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _sequence(rng, steps, max_days):
    """(kind, day) events of one env: an episode's days in order, with skipped days, repeated acts, peeks, forgets and resets"""
    events, d = [("act", 0)], 0
    seen = set()
    while len(events) < steps:
        u = rng.random()
        if u < 0.12:
            events.append(("act", d))               # a second act on the same day
            seen.add("same")
        elif u < 0.24:
            events.append(("peek", d + 1))
            seen.add("peek")
        elif u < 0.32:
            events.append(("forget", d))
            seen.add("forget")
        elif u < 0.44:
            d += int(rng.integers(2, 4))            # days stepped without the agent
            events.append(("act", d))
            seen.add("skip")
        elif d + 1 >= max_days or u < 0.54:
            d = 0                                   # the episode ended: an auto-reset
            events.append(("act", 0))
            seen.add("day0")
        else:
            d += 1
            events.append(("act", d))
    return events, seen


@pytest.mark.parametrize("frames", [1, 2, 3, 8])
@pytest.mark.parametrize("K", [1, 3])
def test_the_twin_equals_the_restatement_over_random_sequences(lib, frames, K):
    rng = np.random.default_rng(100 * frames + K)
    D0, covered = 5 * K + 2, set()
    for trial in range(6):
        ref = S.History(1, K, frames)
        hist, last, frm = np.zeros((frames, D0), F), np.full(1, S.NONE, np.int32), np.zeros(1, np.int32)
        events, seen = _sequence(rng, 60, max_days=2 * frames + 3)
        covered |= seen
        for i, (kind, d) in enumerate(events):
            if kind == "forget":
                ref.forget()
                last[0] = S.NONE
                continue
            f0 = (rng.standard_normal(D0) * 3).astype(F)
            before = (hist.copy(), last.copy(), frm.copy())
            want = ref.row(f0[None], [d], commit=kind == "act")[0]
            got = S.twin_row(lib, K, frames, f0, hist, last, frm, d, kind == "act")
            assert _same(got, want), (trial, i, kind, d)
            if d == 0:
                assert not got[:D0].any(), "frame 0 is zeros on an episode's first day"
            assert _same(hist, ref.hist[0]) and last[0] == ref.last[0] and frm[0] == ref.frm[0], (trial, i, kind, d)
            if kind == "peek":
                assert _same(hist, before[0]) and _same(last, before[1]) and _same(frm, before[2]), "a peek writes nothing"
    assert covered == {"same", "peek", "forget", "skip", "day0"}, covered


def test_the_cases_of_the_law_one_by_one(lib):
    K, frames = 2, 3
    D0 = 5 * K + 2
    rows = [np.full(D0, 10.0 + t, F) for t in range(12)]
    hist, last, frm = np.zeros((frames, D0), F), np.full(1, S.NONE, np.int32), np.zeros(1, np.int32)
    act = lambda t, d, commit=True: S.twin_row(lib, K, frames, rows[t], hist, last, frm, d, commit).reshape(frames, D0)
    zero = np.zeros(D0, F)
    x = act(0, 0)
    assert _same(x, np.stack([zero, zero, zero])) and last[0] == 0 and frm[0] == 0
    x = act(1, 1)
    assert _same(x, np.stack([rows[1], zero, zero])), "day 0's frame is the zeros that act read"
    x = act(2, 2)
    assert _same(x, np.stack([rows[2], rows[1], zero]))
    before = hist.copy()
    x2 = act(2, 2)                                  # a second act on the same day: the same row, the same history
    assert _same(x2, x) and _same(hist, before) and last[0] == 2 and frm[0] == 0
    x = act(3, 3, commit=False)                     # a peek
    assert _same(x, np.stack([rows[3], rows[2], rows[1]])) and _same(hist, before) and last[0] == 2
    x = act(3, 3)
    assert _same(x, np.stack([rows[3], rows[2], rows[1]]))
    x = act(5, 5)                                   # day 4 was stepped without the agent: the history restarts
    assert _same(x, np.stack([rows[5], zero, zero])) and frm[0] == 5
    x = act(6, 6)
    assert _same(x, np.stack([rows[6], rows[5], zero]))
    x = act(7, 0)                                   # an auto-reset: day 0 clears it
    assert _same(x, np.stack([zero, zero, zero])) and frm[0] == 0
    x = act(8, 1)
    assert _same(x, np.stack([rows[8], zero, zero]))
    last[0] = S.NONE                                # an explicit reset's forget; the env is then on day 0 ...
    x = act(9, 0)
    assert _same(x, np.stack([zero, zero, zero]))
    last[0] = S.NONE                                # ... and were it not, nothing older is read
    x = act(10, 4)
    assert _same(x, np.stack([rows[10], zero, zero])) and frm[0] == 4 and last[0] == 4
    # frames = 1: today's row and nothing else
    h1, l1, f1 = np.zeros((1, D0), F), np.full(1, S.NONE, np.int32), np.zeros(1, np.int32)
    assert _same(S.twin_row(lib, K, 1, rows[4], h1, l1, f1, 3, True), rows[4])
    assert not S.twin_row(lib, K, 1, rows[4], h1, l1, f1, 0, True).any()


def test_the_twin_refuses(lib):
    K, D0 = 2, 12
    hist, last, frm, row = np.zeros((9, D0), F), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(9 * D0, F)
    call = lambda frames, day, h=hist: lib.adc_mlp_stack_row_host(K, frames, None, None if h is None else h.ctypes.data, last.ctypes.data,
                                                                    frm.ctypes.data, day, 1, row.ctypes.data)
    assert call(2, 0) == 0
    assert call(0, 0) != 0 and call(9, 0) != 0 and call(2, -1) != 0 and call(2, 0, None) != 0


def test_mlp_policy_frames_validation():
    from adcraft_amd.baselines.mlp_policy import MLPPolicy
    rng = np.random.default_rng(5)
    K = 3
    D0, A = 5 * K + 2, K + 1
    for frames in (1, 2, 3, 8):
        pol = S.random_policy(rng, K, frames, (16, 8), value=True, normalize=True)
        assert pol.frames == frames and pol.num_keywords == K and pol.input_size == frames * D0
        assert pol.shift.shape == (frames * D0,) and pol.log_std.shape == (A,)
        cfg = pol.config(K)
        assert cfg.n_policy_layers == 3 and cfg.policy_widths[2] == A
        with pytest.raises(ValueError, match="inputs"):
            pol.config(K + 1)
    # frames = 1 is the policy it was
    one = R.random_policy(rng, K, (8,))
    assert one.frames == 1 and one.shapes() == ([(D0, 8), (8, A)], [], True, False)
    assert S.random_policy(rng, K, 2, (8,)).shapes() != R.random_policy(rng, 2 * K + 0, (8,)).shapes()
    layers = lambda n_in: [((rng.standard_normal((n_in, 8))).astype(F), np.zeros(8, F)), (rng.standard_normal((8, A)).astype(F), np.zeros(A, F))]
    for bad in (0, 9, -1, 1.5):
        with pytest.raises(ValueError, match="frames"):
            MLPPolicy(layers(2 * D0), frames=bad)
    with pytest.raises(ValueError, match="frames = 2"):
        MLPPolicy(layers(2 * D0 + 1), frames=2)         # a first layer of the wrong width
    with pytest.raises(ValueError, match="frames = 3"):
        MLPPolicy(layers(2 * D0), frames=3)
    with pytest.raises(ValueError, match="inputs"):
        MLPPolicy(layers(2 * D0), frames=2).config(K + 5)
    # the value network reads the same stacked row
    with pytest.raises(ValueError, match="value network"):
        MLPPolicy(layers(2 * D0), frames=2, value_layers=[(rng.standard_normal((D0, 1)).astype(F), np.zeros(1, F))])


def test_random_critics_take_the_stacked_row():
    from adcraft_amd.baselines.td3_trainer import random_critics
    K = 3
    assert random_critics(K, (8,), 0)[0][0][0].shape == (6 * K + 3, 8)
    assert _same(random_critics(K, (8,), 4)[1][0][0], random_critics(K, (8,), 4, frames=1)[1][0][0])
    assert random_critics(K, (8,), 0, frames=4)[0][0][0].shape == (4 * (5 * K + 2) + K + 1, 8)
