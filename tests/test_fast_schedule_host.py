"""CPU: the phase-2 schedule of k_step_implicit_fast through its host twin, adc_fast_schedule_host (adc_shims.cpp), which calls the
schedule helpers of csrc/adc_fast_schedule.h that the kernel calls.  For a tile's volumes the twin lists every (pass, wave, round,
lane) slot the kernel issues with its keyword, first auction and count; the union of the slots must be every auction
0 .. V_k - 1 of every keyword exactly once, and the wave-call-slots issued must stay close to the calls that hold an auction."""
import ctypes as C

import numpy as np
import pytest

from adcraft_amd import synthetic
from oracle import build as obuild

B, WAVE = 256, 64           # lanes of a workgroup, of a wave
VMAX = 1 << 20


@pytest.fixture(scope="module")
def L():
    lib = C.CDLL(obuild.build_shims_host())
    lib.adc_fast_schedule_host.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.adc_fast_schedule_host.restype = C.c_int64
    return lib


def schedule(L, vol, tile_kw=None, tile_index=0):
    vol = np.ascontiguousarray(vol, dtype=np.int32)
    tile_kw = vol.size if tile_kw is None else tile_kw
    totals, info = np.zeros(2, np.int64), np.zeros(2, np.int32)
    n = L.adc_fast_schedule_host(vol.ctypes.data, tile_kw, tile_index, None, 0, totals.ctypes.data, info.ctypes.data)
    assert n >= 0
    rows = np.full((max(n, 1), 7), -7, np.int32)
    assert L.adc_fast_schedule_host(vol.ctypes.data, tile_kw, tile_index, rows.ctypes.data, n, None, None) == n
    return rows[:n], int(totals[0]), int(totals[1]), int(info[0]), int(info[1])


def check_cover(L, vol, tile_kw=None, tile_index=0):
    """every auction of every keyword in exactly one slot, none at or beyond V_k; the slots are well-formed and the issued total is
    the slots' own count"""
    vol = np.asarray(vol, dtype=np.int64)
    rows, issued, needed, shift, dense = schedule(L, vol, tile_kw, tile_index)
    ps, w, r, lane, kw, j0, cnt = (rows[:, i].astype(np.int64) for i in range(7))
    assert ((ps >= 0) & (ps <= 2) & (w >= 0) & (w < B // WAVE) & (lane >= 0) & (lane < WAVE) & (r >= 0)).all()
    assert shift in (2, 3, 4)
    assert shift == (4 if vol.sum() >= 32 * B else 3 if vol.sum() >= 16 * B else 2)
    assert dense == int(vol.sum() >= 24 * (vol > 0).sum())
    busy = cnt > 0
    assert ((kw[~busy] == -1) & (cnt[~busy] == 0)).all()
    assert ((kw[busy] >= 0) & (kw[busy] < vol.size)).all()
    # a slot is one work item: `1 << shift` auctions in pass 0, one call of four in pass 1, one to three auctions in pass 2
    assert (cnt[busy & (ps == 0)] == 1 << shift).all() and (cnt[busy & (ps == 1)] == 4).all() and (cnt[ps == 2] <= 3).all()
    assert (j0[busy] % 4 == 0).all() and (j0[busy] >= 0).all()
    assert (j0[busy] + cnt[busy] <= vol[kw[busy]]).all(), "a slot names an auction at or beyond V_k"
    # (pass, wave, round, lane) names a slot once
    key = ((ps * 4 + w) * (r.max() + 1 if r.size else 1) + r) * WAVE + lane
    assert np.unique(key).size == key.size
    # exact cover: per keyword, the slots' intervals sorted by start tile [0, V_k)
    order = np.lexsort((j0[busy], kw[busy]))
    k_s, a_s, n_s = kw[busy][order], j0[busy][order], cnt[busy][order]
    covered = np.zeros(vol.size, np.int64)
    np.add.at(covered, k_s, n_s)
    assert np.array_equal(covered, vol)
    start = np.ones(k_s.size, bool)
    start[1:] = k_s[1:] != k_s[:-1]
    assert (a_s[start] == 0).all()
    assert (a_s[1:][~start[1:]] == (a_s + n_s)[:-1][~start[1:]]).all(), "auctions covered twice or skipped"
    # wave-call-slots: every (pass, wave, round) that exists issues its item's calls once
    rounds = {(int(a), int(b), int(c)) for a, b, c in zip(ps, w, r)}
    assert issued == sum((1 << shift) // 4 if p == 0 else 1 for p, _, _ in rounds)
    assert needed == int(((vol + 3) // 4).sum())
    assert issued * WAVE >= needed
    return issued, needed


def full(v, n=B):
    return np.full(n, v, np.int64)


def test_all_zero(L):
    rows, issued, needed, _, _ = schedule(L, full(0))
    assert rows.shape[0] == 0 and issued == 0 and needed == 0
    check_cover(L, full(0))


@pytest.mark.parametrize("v", [16, 32])
def test_no_tail(L, v):
    issued, needed = check_cover(L, full(v))
    rows = schedule(L, full(v))[0]
    assert (rows[:, 0] == 0).all()                    # full items only
    assert issued * WAVE == needed                    # and not one empty slot


@pytest.mark.parametrize("v", [15, 17, 3])
def test_uniform_with_tails(L, v):
    check_cover(L, full(v))


def test_chunk_8(L):
    vol = 24 + np.arange(B) % 8
    assert schedule(L, vol)[3] == 3
    check_cover(L, vol)


def test_dense_tile_with_chunk_4(L):
    vol = np.zeros(B, np.int64)
    vol[:100] = 30
    _, _, _, shift, dense = schedule(L, vol)
    assert shift == 2 and dense == 1
    check_cover(L, vol)


@pytest.mark.parametrize("where", [0, 77, 255])
def test_one_keyword_at_the_volume_cap(L, where):
    vol = np.zeros(B, np.int64)
    vol[where] = VMAX
    issued, needed = check_cover(L, vol)
    assert issued * WAVE == needed == VMAX // 4


@pytest.mark.parametrize("partials", [False, True])
@pytest.mark.parametrize("items", [64, 256, 257])
def test_item_totals_at_the_round_edges(L, items, partials):
    """`total` exactly 64 (one wave-round: one wave works), 256 (one round for each wave), 257 (one wave runs a second round).
    (Tiles this small get items of four auctions: 257 items of 8 or 16 would already be a tile of the next item size.)"""
    vol = np.zeros(B, np.int64)
    vol[: min(items, B)] = 4
    vol[0] += 4 * max(items - B, 0)
    if partials:
        vol += np.arange(B) % 4
    rows, _, _, shift, _ = schedule(L, vol)
    assert shift == 2 and int((vol >> shift).sum()) == items
    counts = []
    for tile_index in range(5):         # the four rotations of the waves' parts (and the first again)
        rows = schedule(L, vol, tile_index=tile_index)[0]
        check_cover(L, vol, tile_index=tile_index)
        per_wave = [int(rows[(rows[:, 0] == 0) & (rows[:, 1] == w), 2].max(initial=-1)) + 1 for w in range(B // WAVE)]
        assert sum(per_wave) == -(-items // WAVE) and max(per_wave) - min(per_wave) <= 1
        counts.append(per_wave)
    assert counts[4] == counts[0] and all(counts[t + 1] == counts[t][1:] + counts[t][:1] for t in range(3))


@pytest.mark.parametrize("tile_kw", [256, 64, 16])
def test_random_vectors(L, tile_kw):
    rng = np.random.default_rng(20 + tile_kw)
    for case in range(40):
        kind = case % 4
        if kind == 0:
            vol = rng.integers(0, 300, tile_kw)
        elif kind == 1:
            vol = rng.integers(0, 40, tile_kw) * (rng.random(tile_kw) < 0.5)
        elif kind == 2:
            vol = np.rint(np.clip(128 + 40 * rng.standard_normal(tile_kw), 0, None)).astype(np.int64)
        else:
            vol = (rng.integers(0, 5000, tile_kw) * (rng.random(tile_kw) < 0.1)).astype(np.int64)
        check_cover(L, vol, tile_kw, tile_index=case * 7 + case // 4)


def test_bad_arguments(L):
    v = np.zeros(B, np.int32)
    for tile_kw in (0, -1, B + 1):
        assert L.adc_fast_schedule_host(v.ctypes.data, tile_kw, 0, None, 0, None, None) < 0
    assert L.adc_fast_schedule_host(None, B, 0, None, 0, None, None) < 0
    assert L.adc_fast_schedule_host(v.ctypes.data, B, -1, None, 0, None, None) < 0
    v[3] = -1
    assert L.adc_fast_schedule_host(v.ctypes.data, B, 0, None, 0, None, None) < 0
    v[3] = VMAX + 1
    assert L.adc_fast_schedule_host(v.ctypes.data, B, 0, None, 0, None, None) < 0


def test_issued_over_needed_on_the_cfg2_law(L):
    """64 tiles of the cfg2 law: volumes V = round(clip(vol_mean + vol_std z)) with the planes of
    synthetic.implicit_keyword_planes(512, 256, seed=1729) and z from numpy's default_rng(0) - the statistics of the law, not the
    engine's own stream.  Wave-call-slots issued x 64 over the calls that hold an auction: at most 1.04 in the mean (a schedule that
    still pads every wave to the workgroup's round count, and runs the tail one keyword per lane, gives 1.111)."""
    planes = synthetic.implicit_keyword_planes(512, 256, seed=1729)
    z = np.random.default_rng(0).standard_normal((512, 256))
    x = np.clip(planes[0].astype(np.float64) + planes[1].astype(np.float64) * z, 0.0, float(VMAX))
    V = np.floor(x + 0.5).astype(np.int64)
    ratios = []
    for t in range(64):
        issued, needed = check_cover(L, V[t], tile_index=t)
        ratios.append(issued * WAVE / needed)
    mean = float(np.mean(ratios))
    print(f"mean volume {V[:64].mean():.1f}; issued / needed: mean {mean:.4f}, max {max(ratios):.4f}")
    assert mean <= 1.04
