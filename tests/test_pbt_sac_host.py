"""-m "not gpu": the SAC kind (ADC_PBT_SAC = 3) of the population-based training scheduler on the host - adc_pbt_explore_host
against the numpy restatement tests/pbt_sac_ref.py bit for bit, every kind-3 refusal and legal corner of adc_pbt_config_check,
StepEngine.pbt_config("sac") and the new entry point's declaration, export and binding.  Neither the kind nor the symbol exists
before this feature: every test here fails on the parent commit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import pbt_ref as B
from tests import pbt_sac_ref as BS

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = {"actor_lr": (1e-5, 1e-2), "critic_lr": (1e-5, 1e-2), "alpha_lr": (0.0, 1e-2), "tau": (1e-3, 0.5), "alpha": (0.05, 2.0),
          "target_entropy": (-12.0, -0.5)}


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _config(members=8, replace_count=2, **kw):
    from adcraft_amd.engine import StepEngine
    return StepEngine.pbt_config("sac", members, replace_count, **kw)


def test_the_kind_and_its_ids():
    from adcraft_amd import _ffi
    from adcraft_amd.engine import StepEngine
    assert _ffi.PBT_SAC == BS.SAC == 3 and StepEngine.PBT_KINDS["sac"] == 3
    assert StepEngine.PBT_IDS["sac"] == BS.SAC_IDS and len(BS.SAC_IDS) == 6 and BS.SAC_IDS[BS.ALPHA] == "alpha"
    assert StepEngine.PBT_IDS["td3"][BS.ALPHA] == "sigma", "id 4 is the device-side, log-domain one for both kinds"
    assert (_ffi.PBT_PG, _ffi.PBT_TD3) == (0, 1)


def test_explore_every_id_both_factors_and_both_bounds(lib):
    own = np.array([0.123, 0.5, 0.3, 0.7, -1.0, -4.0, 9.0, 9.0], F)
    for h, name in enumerate(BS.SAC_IDS):
        c = _config(tuned=(name,), bounds=BOUNDS, factors=(0.8, 1.25))
        cfg = B.config_dict(c)
        lo, hi = cfg["lo"][h], cfg["hi"][h]
        span = [lo, hi, np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf)), F(lo * F(1.2)), F(hi * F(0.9)), F(lo - F(3)), F(hi + F(3)),
                F((lo + hi) / 2), F(0.0), F(-0.0)]
        for v in span:
            donor = np.array([7.0] * 8, F)
            donor[h] = v
            for bits in (0, 1 << h, 0xFFFFFFFF, 0xFFFFFFFF ^ (1 << h)):
                got, ref = B.twin_explore(lib, c, BS.SAC, bits, donor, own), BS.explore(cfg, bits, donor, own)
                assert _same(got, ref), (name, v, bits)
                others = [i for i in range(8) if i != h]
                assert _same(got[others], own[others]), "ids outside the mask keep the member's own value"
                if h == BS.ALPHA:
                    assert _same(got[h], own[h]), "the temperature is left to the device: the host explore passes the member's own through"
                else:
                    assert lo <= got[h] <= hi
        if h == BS.ALPHA:
            continue
        # both factors are reached, and differ, inside the bounds; both clamps fire outside them
        mid = np.array([F((lo + hi) / 2)] * 8, F)
        down, up = B.twin_explore(lib, c, BS.SAC, 0, mid, own)[h], B.twin_explore(lib, c, BS.SAC, 1 << h, mid, own)[h]
        assert _same(down, F(mid[h] * F(0.8))) and _same(up, F(mid[h] * F(1.25))) and down != up
        below, above = np.array([F(lo - F(3))] * 8, F), np.array([F(hi + F(3))] * 8, F)
        if name == "target_entropy":
            # negative values: the larger factor moves further from 0, so it is the one that can fall below lo
            assert mid[h] < 0 and up < mid[h] < down
            assert _same(B.twin_explore(lib, c, BS.SAC, 1 << h, below, own)[h], lo) and _same(B.twin_explore(lib, c, BS.SAC, 0, above, own)[h], hi)
        else:
            assert down < mid[h] < up
            assert _same(B.twin_explore(lib, c, BS.SAC, 0, below, own)[h], lo) and _same(B.twin_explore(lib, c, BS.SAC, 1 << h, above, own)[h], hi)
    # all ids at once
    c = _config(tuned=BS.SAC_IDS, bounds=BOUNDS)
    donor = np.array([3e-4, 1e-3, 2e-3, 0.01, -2.0, -6.0, 0, 0], F)
    for bits in range(64):
        got = B.twin_explore(lib, c, BS.SAC, bits, donor, own)
        assert _same(got, BS.explore(B.config_dict(c), bits, donor, own)), bits
        assert _same(got[BS.ALPHA], own[BS.ALPHA]) and got[5] < 0
    # kind 2 stays unassigned
    out = np.zeros(8, F)
    assert lib.adc_pbt_explore_host(C.byref(c), 2, 0, donor.ctypes.data, own.ctypes.data, out.ctypes.data) != 0


def test_the_restated_cell_and_round():
    """the restatement's own consistency: the cell's shift and clamp, a replaced member's smoothed fitness and hp[4]"""
    c = _config(tuned=("alpha", "actor_lr"), bounds=BOUNDS, factors=(0.5, 2.0), fitness_ema=0.5)
    cfg = B.config_dict(c)
    lo, hi = cfg["lo"][4], cfg["hi"][4]
    assert _same(lo, F(np.log(0.05))) and _same(hi, F(np.log(2.0)))
    la3 = np.array([-1.0, 0.25, 0.5], F)
    down, a_down = BS.cell_after(cfg, 0, la3)
    up, a_up = BS.cell_after(cfg, 1 << 4, la3)
    assert _same(down[0], F(F(-1.0) + F(np.log(0.5)))) and _same(up[0], F(F(-1.0) + F(np.log(2.0))))
    assert _same(down[1:], la3[1:]) and _same(up[1:], la3[1:]), "the moments are the donor's"
    assert a_down < np.exp(-1.0) < a_up
    assert _same(BS.cell_after(cfg, 0, [-2.9, 0, 0])[0][0], lo) and _same(BS.cell_after(cfg, 1 << 4, [0.5, 0, 0])[0][0], hi)
    untuned = B.config_dict(_config(tuned=("actor_lr",), bounds=BOUNDS))
    assert _same(BS.cell_after(untuned, 1 << 4, la3)[0], la3) and BS.shift_of(untuned, 1 << 4) == 0
    hp = BS.hp_of([dict(actor_lr=1e-3 * (m + 1), critic_lr=1e-3, alpha_lr=0.0, tau=0.01, target_entropy=-3.0) for m in range(8)])
    state = dict(round=0, smoothed=np.zeros(8))
    for r in range(3):
        state, res = BS.round_(cfg, 11, state, np.random.default_rng(r).standard_normal(8), hp)
        for m in range(8):
            if res["src"][m] >= 0:
                assert res["smoothed"][m] == res["smoothed"][res["src"][m]]
                assert res["hp"][m, 4] in (F(np.log(0.5)), F(np.log(2.0)))
            else:
                assert _same(res["hp"][m, list(BS.HOST_IDS)], hp[m, list(BS.HOST_IDS)]) and res["hp"][m, 4] == 0
        hp = res["hp"]
    assert state["round"] == 3


def _check(lib, c, members=8, kind=BS.SAC):
    msg = C.c_char_p()
    rc = lib.adc_pbt_config_check(C.byref(c), members, kind, C.byref(msg))
    return rc, (msg.value or b"").decode()


def _good():
    return _config(tuned=("tau", "alpha", "alpha_lr"), bounds=BOUNDS)


def _bound(h, lo, hi):
    def change(c):
        c.tuned_mask |= 1 << h
        c.lo[h], c.hi[h] = lo, hi
    return change


def test_config_check_refusals(lib):
    from adcraft_amd import _ffi

    def refused(change, word=""):
        c = _good()
        change(c)
        rc, msg = _check(lib, c)
        assert rc == _ffi.ADC_EINVAL and word in msg, (rc, msg, word)

    assert _check(lib, _good()) == (0, "")
    refused(lambda c: setattr(c, "tuned_mask", 1 << 6), word="tuned_mask")
    refused(lambda c: setattr(c, "tuned_mask", c.tuned_mask | (1 << 7)), word="tuned_mask")
    refused(lambda c: setattr(c, "with_ring", 2), word="with_ring")
    refused(_bound(3, 0.0, 0.5), word="tau")
    refused(_bound(3, 1e-3, 1.5), word="tau")
    for h in (0, 1, 2):
        refused(_bound(h, -1e-5, 1e-2), word="at least 0")
    for h in range(6):
        lo, hi = (0.2, 0.1) if h < 4 else (-1.0, -2.0)
        refused(_bound(h, lo, hi), word="lo <= hi")
        refused(_bound(h, float("nan"), 0.5), word="lo")
        refused(_bound(h, 1e-3, float("nan")), word="hi")
        refused(_bound(h, 1e-3, float("inf")), word="finite")
        refused(_bound(h, float("-inf"), 0.5), word="finite")
    # what does not depend on the kind is refused for it too
    refused(lambda c: setattr(c, "replace_count", 5), word="replace_count")
    refused(lambda c: setattr(c, "log_factor_lo", float("nan")), word="log_factor")
    # kind 2 is unassigned
    rc, msg = _check(lib, _good(), kind=2)
    assert rc == _ffi.ADC_EINVAL and "kind" in msg


def test_config_check_legal_corners(lib):
    def accepted(change):
        c = _good()
        change(c)
        assert _check(lib, c) == (0, ""), _check(lib, c)

    accepted(lambda c: setattr(c, "with_ring", 1))
    accepted(_bound(4, -5.0, -1.0))                 # log_alpha bounds: alpha below 1
    accepted(_bound(4, -1.0, 1.0))
    accepted(_bound(5, -20.0, -0.5))                # a negative target entropy is the usual one
    accepted(_bound(5, -3.0, 3.0))
    accepted(_bound(2, 0.0, 0.0))                   # alpha_lr 0: the temperature stays
    accepted(_bound(3, 1e-3, 1.0))                  # tau 1 is legal
    # all six ids tuned at once
    c = _good()
    c.tuned_mask = 0x3F
    for h, name in enumerate(BS.SAC_IDS):
        c.lo[h], c.hi[h] = (F(np.log(BOUNDS[name][0])), F(np.log(BOUNDS[name][1]))) if name == "alpha" else BOUNDS[name]
    assert _check(lib, c) == (0, "")
    # an untuned id's bounds are not read
    c = _good()
    c.lo[0], c.hi[0] = 5.0, -5.0
    c.lo[5], c.hi[5] = float("nan"), float("inf")
    assert _check(lib, c) == (0, "")
    # every admitted bound is a value adc_sac_config_check admits in that field
    from adcraft_amd.engine import StepEngine
    for name, values in (("tau", (np.nextafter(F(0), F(1)), 1.0)), ("actor_lr", (0.0, 3e38)), ("critic_lr", (0.0, 3e38)), ("alpha_lr", (0.0, 3e38)),
                         ("target_entropy", (-3e38, 3e38))):
        for v in values:
            StepEngine.sac_config(num_keywords=5, **{name: float(v)})


def test_python_config_fills_the_log_bounds_of_alpha():
    c = _config(tuned=("alpha",), bounds={"alpha": (0.05, 2.0)}, factors=(0.5, 2.0), with_ring=True)
    assert _same(F(c.log_factor_lo), F(np.log(0.5))) and _same(F(c.log_factor_hi), F(np.log(2.0)))
    assert _same(F(c.lo[4]), F(np.log(0.05))) and _same(F(c.hi[4]), F(np.log(2.0)))
    assert c.tuned_mask == 1 << 4 and c.with_ring == 1
    c = _config(tuned=("target_entropy", "alpha_lr"), bounds=BOUNDS)
    assert c.tuned_mask == (1 << 5) | (1 << 2) and _same(F(c.lo[5]), F(-12.0)) and _same(F(c.hi[5]), F(-0.5)), "linear bounds are stored as given"
    for bad in ((0.0, 2.0), (-0.5, 2.0), (0.05, 0.0), (0.05, -1.0)):
        with pytest.raises(ValueError, match="alpha"):
            _config(tuned=("alpha",), bounds={"alpha": bad})
    with pytest.raises(ValueError):
        _config(tuned=("sigma",), bounds={"sigma": (0.01, 1.0)})
    with pytest.raises(ValueError):
        _config(tuned=("alpha",))
    with pytest.raises(ValueError):
        _config(tuned=("tau",), bounds={"tau": (0.0, 0.5)})
    from adcraft_amd.engine import StepEngine
    with pytest.raises(ValueError):
        StepEngine.pbt_config("pg", 8, 2, tuned=("alpha",), bounds={"alpha": (0.05, 2.0)})


def test_the_new_entry_point_is_declared_exported_and_bound(lib):
    from adcraft_amd import _ffi
    header = open(os.path.join(ROOT, "include", "adcraft_engine.h")).read()
    assert re.search(r"\bint\s+adc_engine_pbt_init_sac\s*\(\s*adc_engine\s*\*\s*e\s*,\s*const\s+adc_pbt_config\s*\*\s*cfg\s*\)\s*;", header)
    assert re.search(r"ADC_PBT_PG\s*=\s*0\s*,\s*ADC_PBT_TD3\s*=\s*1\s*,\s*ADC_PBT_SAC\s*=\s*3\b", header)
    assert "#define ADC_ABI_VERSION 5" in header or re.search(r"ADC_ABI_VERSION\s+5\b", header), "the ABI version stays 5"
    fn = lib.adc_engine_pbt_init_sac
    assert fn.restype is C.c_int and len(fn.argtypes) == 2 and fn.argtypes[1] == C.POINTER(_ffi.PBTConfig)
    raw = C.CDLL(lib._name)
    assert C.cast(raw.adc_engine_pbt_init_sac, C.c_void_p).value, "the library exports the symbol"
    # a NULL engine is refused before anything is touched
    assert fn(None, C.byref(_good())) == _ffi.ADC_EINVAL
