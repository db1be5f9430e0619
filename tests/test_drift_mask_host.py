"""Partial updater masks without a GPU: the reference's rule for which keywords update_keywords() moves (SURVEY B-6,
gymnasium_kw_env.py:130-144) as gymnasium_kw_utils.effective_updater_mask, on hand cases and on G14 (recorded from the
reference itself); a numpy restatement of the masked update on G14's own vectors; the facade's constructor and
set_updater_mask on partial masks."""
import numpy as np
import pytest

from adcraft_amd import gymnasium_kw_utils as utils
from adcraft_amd.gymnasium_kw_env import BiddingSimulation

T, F = True, False


def test_effective_mask_hand_cases():
    e = utils.effective_updater_mask
    assert e(None) is None
    assert e([T, F, T, T, F, T]).tolist() == [T, F, T, T, F, F]          # keyword 5 lies beyond sum(mask) = 4
    assert e([F, F, F, T, F, F]).tolist() == [F] * 6                      # sum 1: only keyword 0 is visited, and it is masked
    assert e([T] * 5).tolist() == [T] * 5
    assert e([F] * 5).tolist() == [F] * 5
    assert e([T, F] * 4).tolist() == [T, F, T, F, F, F, F, F]
    assert e([F, T, T, T]).tolist() == [F, T, T, F]
    rows = e(np.array([[T, F, T, T, F, T], [F, T, F, F, F, F], [T] * 6]))
    assert rows.shape == (3, 6) and rows.dtype == bool
    assert rows.tolist() == [[T, F, T, T, F, F], [F] * 6, [T] * 6]          # row 1: sum 1, keyword 0 is masked
    with pytest.raises(ValueError):
        e(np.zeros((2, 2, 2), bool))


def _moved(a, b):
    return [bool(x) for x in (np.asarray(a) != np.asarray(b)).any(axis=1)]


def _vol_ctr_cvr(params):
    return np.array([[p[0][0], p[3], p[4]] for p in params], dtype=np.float64)


def test_effective_mask_on_g14(golden):
    """the keywords the reference moved at every recorded update are exactly the effective selection's"""
    d = golden("g14_partial_updater_mask.json")
    names = {c["name"] for c in d["cases"]}
    assert {"beyond_prefix", "only_beyond_prefix", "alternating", "all_false", "set_between"} <= names
    for c in d["cases"]:
        prev = _vol_ctr_cvr(c["params0"])
        for st in c["steps"]:
            eff = utils.effective_updater_mask(st["mask"])
            assert st["num_updates"] == sum(st["mask"])
            assert all(len(u) == st["num_updates"] for u in st["uniforms"])
            cur = _vol_ctr_cvr(st["params"])
            moved = _moved(prev, cur)
            # a selected keyword can stay put only if all three of its coefficients left it unchanged (never in G14)
            assert moved == eff.tolist(), (c["name"], st["mask"])
            prev = cur


def test_numpy_restatement_of_g14(golden):
    """the recorded vectors applied to the selected keywords (the k-th entry to keyword k) give G14's parameters:
    vol_mean += u_vol * vol_std clipped at 0, bctr *= 1 + u_ctr and sctr *= 1 + u_cvr clipped to [0, 1]
    (gymnasium_kw_env.py:146-158), in float64 as the reference holds them"""
    d = golden("g14_partial_updater_mask.json")
    for c in d["cases"]:
        p = [[list(q[0])] + list(q[1:]) for q in c["params0"]]
        vol_std = [q[0][1] for q in c["params0"]]          # init_volumes: the volume std at the first update
        for st in c["steps"]:
            eff = utils.effective_updater_mask(st["mask"])
            uv, uc, us = st["uniforms"]
            for k in np.flatnonzero(eff):
                p[k][0][0] = max(p[k][0][0] + uv[k] * vol_std[k], 0.0)
                p[k][3] = min(max(p[k][3] * (1 + uc[k]), 0.0), 1.0)
                p[k][4] = min(max(p[k][4] * (1 + us[k]), 0.0), 1.0)
            for k, q in enumerate(st["params"]):
                assert p[k][0][0] == q[0][0] and p[k][0][1] == q[0][1], (c["name"], k)
                assert p[k][3] == q[3] and p[k][4] == q[4], (c["name"], k)
                assert p[k][1:3] == q[1:3] and p[k][5:] == q[5:]


def test_facade_accepts_partial_masks_without_a_gpu():
    env = BiddingSimulation(num_keywords=6, updater_mask=[T, F, T, T, F, T])
    assert env.num_updates == 4
    assert env.updater_mask == [T, F, T, T, F, T]
    assert env._effective_mask.tolist() == [T, F, T, T, F, F] and env._drift_on()
    env.set_updater_mask([F, F, F, T, F, F])              # selects nothing: drift stays off
    assert env.num_updates == 1 and not env._drift_on()
    env.set_updater_mask([F] * 6)
    assert env.num_updates == 0 and not env._drift_on()
    env.set_updater_mask([T] * 6)
    assert env.num_updates == 6 and env._drift_on()
    assert BiddingSimulation(num_keywords=3)._effective_mask is None


def test_wrong_length_mask_fails_the_reference_assertion():
    with pytest.raises(AssertionError):
        BiddingSimulation(num_keywords=6, updater_mask=[T, F, T])         # gymnasium_kw_env.py:107-110
    env = BiddingSimulation(num_keywords=4)
    with pytest.raises(AssertionError):
        env.set_updater_mask([T, F, T, T, F])
