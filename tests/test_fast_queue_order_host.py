"""CPU: the protocol of k_step_implicit_fast's per-wave queue of clicked wins, with the move-down ahead of the batch's resolution.

A push writes the lanes of a 64-bit mask behind the entries that wait; whenever 64 or more wait, a drain reads the batch [0, 64) into
registers, reads the entries behind it, writes those to [0, 64) with all 64 lanes, takes 64 off the fill and only then resolves the
batch from the registers; what is left at the end is one partial batch.  adc_fast_queue_host (csrc/shims/fast_pass.inc) runs that
protocol, one LDS instruction of the wave after the other, and reports what every batch resolved.  Over random and hand-made mask
sequences the batches together hold every pushed entry exactly once and each holds 64 entries except the last; the same model with
the move-down's write ahead of the batch read does not (the check can fail).  Host build of the shims (g++)."""
import ctypes as C

import numpy as np
import pytest

from oracle import build as obuild

FREE = 0xFFFFFFFF          # what a slot holds that no push has written
N_SEQUENCES = 10_000       # per density
DENSITIES = [0.02, 0.28, 0.9, 1.0]
ALL = (1 << 64) - 1


@pytest.fixture(scope="module")
def L():
    lib = C.CDLL(obuild.build_shims_host())
    vp = C.c_void_p
    lib.adc_fast_queue_host.argtypes = [vp, C.c_int64, C.c_int32, vp, C.c_int64, vp, C.c_int64, vp]
    lib.adc_fast_queue_host.restype = C.c_int64
    return lib


def _run(L, masks, write_first=0):
    """-> (entries resolved, in batch order; rows {entries waiting at the batch, entries it resolved}; {pushed, largest fill})"""
    masks = np.ascontiguousarray(masks, dtype=np.uint64)
    pushed = int(np.unpackbits(masks.view(np.uint8)).sum())
    entries = np.full(pushed + 128, 0xABABABAB, np.uint32)
    batches = np.zeros((pushed // 64 + 2, 2), np.int32)
    info = np.zeros(3, np.int64)
    n = L.adc_fast_queue_host(masks.ctypes.data, masks.size, write_first, entries.ctypes.data, entries.size, batches.ctypes.data,
                              batches.shape[0], info.ctypes.data)
    assert n >= 0, n
    assert n <= entries.size and info[0] <= batches.shape[0]
    return entries[:n], batches[:info[0]], dict(pushed=int(info[1]), max_fill=int(info[2]))


def _expected(masks):
    """the entries a sequence pushes, ascending: push index << 6 | lane"""
    bits = np.unpackbits(np.ascontiguousarray(masks, dtype=np.uint64).view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")
    return np.flatnonzero(bits).astype(np.uint32)


def _problems(masks, entries, batches, info):
    """what is wrong with a run, as a list of words (empty: the protocol held)"""
    want = _expected(masks)
    bad = []
    if info["pushed"] != want.size:
        bad.append("pushed")
    if info["max_fill"] > 63 + 64:
        bad.append("fill")
    if entries.size != want.size or not np.array_equal(np.sort(entries), want):
        bad.append("entries")          # (sorted and equal to a strictly ascending list: each exactly once)
    sizes = batches[:, 1]
    if sizes.sum() != entries.size or (sizes[:-1] != 64).any() or (sizes.size and not 1 <= sizes[-1] <= 64):
        bad.append("sizes")
    if sizes.size != (want.size + 63) // 64:
        bad.append("batches")
    if sizes.size > 1 and (batches[:-1, 0] < 64).any():
        bad.append("early drain")
    return bad


def _random_sequences(rng, density, count):
    """`count` sequences of up to ~320 entries each, as one array of masks and the sequences' bounds in it"""
    longest = max(2, int(np.ceil(320.0 / (64.0 * density))))
    lengths = rng.integers(1, longest + 1, count)
    bounds = np.concatenate([[0], np.cumsum(lengths)])
    bits = rng.random((int(bounds[-1]), 64), dtype=np.float32) < density
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).ravel(), bounds


@pytest.mark.parametrize("density", DENSITIES)
def test_random_sequences_resolve_every_entry_once(L, density):
    rng = np.random.default_rng(int(density * 100) + 5)
    drains = 0
    for _ in range(N_SEQUENCES // 1000):
        masks, bounds = _random_sequences(rng, density, 1000)
        for a, b in zip(bounds[:-1], bounds[1:]):
            m = masks[a:b]
            entries, batches, info = _run(L, m)
            assert _problems(m, entries, batches, info) == [], (density, [hex(int(x)) for x in m])
            drains += max(len(batches) - 1, 0)
    assert drains > N_SEQUENCES // 2          # the sequences did reach the move-down


def _mask(n, first=0):
    return ((1 << n) - 1) << first


# hand-made sequences, by the entries that wait when a drain starts
HAND = {
    "exactly-64": [_mask(40), _mask(24, 40)],
    "exactly-65": [_mask(40), _mask(25, 3)],
    "exactly-127": [_mask(63), ALL],
    "63-plus-64-then-more": [_mask(63, 1), ALL, _mask(1, 63), ALL, ALL],
    "push-of-no-lane": [_mask(30), 0, _mask(34, 30), 0, 0, _mask(5)],
    "ends-empty": [ALL, ALL, _mask(32), _mask(32, 32)],
    "nothing-pushed": [0, 0, 0],
    "one-left": [ALL, _mask(1, 17)],
    "scattered": [0x8000000000000001, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 0xF0F0F0F0F0F0F0F0, 0x00000000FFFFFFFF, 0x8000000000000000],
}
FILLS = {"exactly-64": [64], "exactly-65": [65, 1], "exactly-127": [127, 63], "63-plus-64-then-more": [127, 64, 64, 64],
         "push-of-no-lane": [64, 5], "ends-empty": [64, 64, 64], "nothing-pushed": [], "one-left": [64, 1]}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_sequences(L, name):
    m = np.array(HAND[name], np.uint64)
    entries, batches, info = _run(L, m)
    assert _problems(m, entries, batches, info) == []
    if name in FILLS:
        assert batches[:, 0].tolist() == FILLS[name]
    if name == "ends-empty":
        assert batches[:, 1].tolist() == [64, 64, 64]          # the last batch is a full one: no partial batch follows
    # a drain resolves the oldest 64: the first batch is the first 64 entries pushed, in their order
    if len(batches):
        assert np.array_equal(entries[:batches[0, 1]], _expected(m)[:batches[0, 1]])


def test_write_before_the_batch_read_fails_the_check(L):
    """the move-down's write ahead of the batch read overwrites entries no lane has read: the same check then fails, wherever
    a drain runs"""
    for name in ("exactly-65", "exactly-127", "63-plus-64-then-more", "scattered"):
        m = np.array(HAND[name], np.uint64)
        assert "entries" in _problems(m, *_run(L, m, write_first=1)), name
    rng = np.random.default_rng(77)
    failed = checked = 0
    for density in DENSITIES:
        masks, bounds = _random_sequences(rng, density, 200)
        for a, b in zip(bounds[:-1], bounds[1:]):
            m = masks[a:b]
            good = _run(L, m)
            if (good[1][:, 1] == 64).any():          # a drain ran (the last, partial batch holds fewer than 64)
                checked += 1
                failed += "entries" in _problems(m, *_run(L, m, write_first=1))
            else:                                    # no drain, no move-down: the two orders are the same run
                assert _problems(m, *_run(L, m, write_first=1)) == []
    assert checked > 100 and failed == checked
    # with nothing behind the batch it is free slots that the write brings down over it
    m = np.array(HAND["exactly-64"], np.uint64)
    assert (_run(L, m, write_first=1)[0] == FREE).all()


def test_arguments(L):
    e, b, i = np.zeros(4, np.uint32), np.zeros((2, 2), np.int32), np.zeros(3, np.int64)
    m = np.array([ALL], np.uint64)
    assert L.adc_fast_queue_host(None, 1, 0, e.ctypes.data, 4, b.ctypes.data, 2, i.ctypes.data) < 0
    assert L.adc_fast_queue_host(m.ctypes.data, -1, 0, e.ctypes.data, 4, b.ctypes.data, 2, i.ctypes.data) < 0
    assert L.adc_fast_queue_host(m.ctypes.data, 1, 2, e.ctypes.data, 4, b.ctypes.data, 2, i.ctypes.data) < 0
    # outputs shorter than the result: the count is returned, the first `cap` are written
    assert L.adc_fast_queue_host(m.ctypes.data, 1, 0, e.ctypes.data, 4, b.ctypes.data, 2, i.ctypes.data) == 64
    assert e.tolist() == [0, 1, 2, 3] and i.tolist() == [1, 64, 64] and b[0].tolist() == [64, 64]
    assert L.adc_fast_queue_host(m.ctypes.data, 1, 0, None, 0, None, 0, None) == 64
