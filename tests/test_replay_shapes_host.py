"""The host twins against the numpy restatements at the shapes of tests/replay_shapes.py, so that what
tests/test_gpu_replay_shapes.py holds the device to is itself checked where no device is needed: the n-step windows of a
record of 5 days x 6 envs through an auto-reset, the prioritised-replay tree, its sampler and its leaf update at capacity
4200 (three levels), the observation and reward normalisers at 1050 samples (two chunks, the second starting inside a day)
and 262 columns, and the last K the off-policy learners' LDS limit accepts with 8 frames against a scan of the restated count."""
import numpy as np
import pytest

from tests import learner_shapes as W
from tests import norm_ref as NR
from tests import nstep_ref as NS
from tests import per_ref as PR
from tests import replay_shapes as RS
from tests import rew_norm_ref as RR
from tests import td3_norm_ref as TN

F, D64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 1. the windows -------------------------------------------------------------------------------------------------------------------
def _record(rng, first_day, T=RS.STORE["T"], N=RS.STORE["N"], max_days=RS.RESETS["max_days"]):
    """a record as the engine leaves it under max_days with auto-reset, from episode day `first_day`: every env is truncated on its
    episode's last day; env 1 also terminates a day early once"""
    reward = (rng.standard_normal((T, N)) * 3).astype(F)
    day = (first_day + np.arange(T)) % max_days
    truncated = np.repeat((day == max_days - 1)[:, None], N, axis=1)
    terminated = np.zeros((T, N), bool)
    terminated[int(np.flatnonzero(day == max_days - 2)[0]), 1] = True
    return dict(reward=reward, terminated=terminated, truncated=truncated)


@pytest.mark.parametrize("first_day", [0, 1], ids=["first-store", "second-store"])
@pytest.mark.parametrize("n", [3, 1])
def test_windows_of_the_store_cases_equal_the_restatement(lib, n, first_day):
    rec = _record(np.random.default_rng(10 + first_day), first_day)
    w, reach = RS.store_windows(f"host windows n={n} first_day={first_day}", rec, n)
    got = NS.twin_windows(lib, n, RS.STORE["gamma"], rec["reward"], rec["terminated"], rec["truncated"])
    for k in ("R", "done", "gn", "m"):
        assert _same(got[k], w[k]), k
    if n > 1:
        assert not _same(w["R"], rec["reward"].reshape(-1)) and len(set(w["gn"].tolist())) == n
    # a fragment [t0, t1) inside the record, as a second store of the same record takes it
    part = NS.windows(n, RS.STORE["gamma"], rec["reward"], rec["terminated"], rec["truncated"], 2, 4)
    got = NS.twin_windows(lib, n, RS.STORE["gamma"], rec["reward"], rec["terminated"], rec["truncated"], 2, 4)
    for k in ("R", "done", "gn", "m"):
        assert _same(got[k], part[k]), k


# ---- 2. the tree on three levels ------------------------------------------------------------------------------------------------------
def test_tree_sampler_and_leaf_update_at_capacity_4200(lib):
    C_, B, top = RS.TREE["C"], RS.TREE["B"], RS.TREE["top"]
    assert RS.tree_shape(C_) == [4200, 66, 2, 1]
    leaf = RS.tree_leaves(2)
    ref = PR.Tree(C_, leaf, top=top)
    L, counts, nodes = PR.twin_tree(lib, C_, leaf)
    assert L == 3 and list(counts) == ref.n and _same(nodes, ref.nodes())
    rng = np.random.default_rng(3)
    for update in (0, 1, 2):
        idx, w = PR.twin_sample(lib, C_, C_, ref.leaf[:C_], 123, update, B, beta=0.4)
        ridx, rw = PR.sample(ref, 123, update, B, C_, 0.4)
        assert _same(idx, ridx) and _same(w, rw), update
        RS.tree_batch(f"host tree update {update}", ridx)
        # new priorities for the batch: the maximum over a slot's duplicates, top, and the nodes of every level above the slots
        pab = (10.0 ** rng.uniform(-2, 2.5, B)).astype(F)
        lf, t = PR.twin_leaf_update(lib, C_, ref.leaf[:C_], ref.top, ridx, pab)
        before = ref.nodes().copy()
        PR.leaf_update(ref, ridx, pab)
        assert _same(lf, ref.leaf[:C_]) and _same(t, F(ref.top)), update
        L, counts, nodes = PR.twin_tree(lib, C_, lf)
        assert _same(nodes, ref.nodes()), "the paths' rebuild gives the nodes of a whole rebuild"
        assert not _same(before[66:], ref.nodes()[66:]), "the levels above the first moved"
    assert ref.top > F(top)
    # a wrapping store's slots: two ranges under different level-1 and level-2 nodes
    ref.fill([(4190 + s) % C_ for s in range(16)])
    whole = PR.Tree(C_, ref.leaf[:C_], top=ref.top)
    assert _same(whole.nodes(), ref.nodes()) and np.all(ref.leaf[4190:4200] == ref.top) and np.all(ref.leaf[:6] == ref.top)


# ---- 3. the normalisers at 1050 samples and 262 columns -----------------------------------------------------------------------------
def _rows(rng, S, D):
    x = (rng.standard_normal((S, D)) * (1.0 + np.arange(D) % 7) + np.arange(D) % 5).astype(F)
    x[::7] = 0                                                     # (an episode's first day)
    return x


def _columns(state, cols):
    return dict(count=state["count"], **{k: np.ascontiguousarray(state[k][cols]) for k in ("mean", "M2", "shift", "scale")})


def test_observation_twins_at_two_chunks_and_two_column_tiles(lib):
    K, n, T = RS.NORM["K"], RS.NORM["n"], RS.NORM["T"]
    S, D, cols = n * T, 5 * K + 2, list(RS.NORM["cols"])
    assert (S, D) == (1050, 262) and RS.norm_shape("host observation rows", S, D, n) == [1024, 26]
    rng = np.random.default_rng(4)
    shift, scale = (rng.random(D) * 3).astype(F), (0.01 + rng.random(D) * 0.2).astype(F)
    for fresh, update, twin in ((NR.fresh, NR.update, NR.twin), (TN.obs_fresh, TN.obs_update, TN.twin_obs)):
        ref = got = fresh(D, shift, scale)
        for rnd in range(2):                                       # (the second merges into count > 0)
            x = _rows(rng, S, D)
            part = update(_columns(ref, cols), x[:, cols])       # (the law is column by column: the four columns alone)
            ref, got = update(ref, x), twin(lib, got, x)
            assert NR.same(got, ref), rnd
            for k in ("mean", "M2", "shift", "scale"):
                assert _same(got[k][cols], part[k]), (k, rnd)
        assert ref["count"] == 2 * S and np.all(ref["scale"][cols] != scale[cols])


def test_reward_twin_at_two_chunks(lib):
    n, T = RS.NORM["n"], RS.NORM["T"]
    rng = np.random.default_rng(5)
    ref = got = RR.fresh(n)
    for rnd in range(2):
        reward = (rng.standard_normal((T, n)) * 3).astype(F)
        day = (rnd * T + np.arange(T)) % 7
        truncated = np.repeat((day == 6)[:, None], n, axis=1)
        terminated = rng.random((T, n)) < 0.02
        ref = RR.update(ref, reward, terminated, truncated, F(0.97))
        got = RR.twin(lib, got, reward, terminated, truncated, F(0.97))
        assert RR.same(got, ref), rnd
    assert ref["count"] == 2 * n * T and ref["scale"] != F(1.0) and np.any(ref["returns"] != 0)


# ---- 4. the off-policy learners' last K with frames --------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,frames,by_hand", [("td3", 8, 329), ("sac", 8, 255), ("td3", 1, 1483), ("sac", 1, 702)])
def test_boundary_k_with_frames_equals_a_scan_of_the_restated_count(family, frames, by_hand):
    """by hand at 8 frames under hidden (256, 256, 256) and critics (256, 256, 256, 1): TD3 holds 45 K + 1562 floats for K >= 255,
    SAC 55 K + 2345"""
    fits = [K for K in range(1, 2000) if W.widest_count(family, K, frames) <= W.LDS_FLOATS]
    assert fits == list(range(1, fits[-1] + 1)), "the count grows with K"
    K = W.boundary_K(family, frames)
    RS.log(f"host boundary {family} frames={frames}", K=K, floats_at_K=W.widest_count(family, K, frames), floats_at_K_plus_1=W.widest_count(family, K + 1, frames),
           limit=W.LDS_FLOATS)
    assert K == fits[-1] == by_hand
    if frames == 8:
        line = (lambda k: 45 * k + 1562) if family == "td3" else (lambda k: 55 * k + 2345)
        assert all(W.widest_count(family, k, 8) == line(k) for k in range(255, 400))
        assert W.widest_count(family, K + 1, 1) <= W.LDS_FLOATS, "one frame of K + 1 fits: the frames are to blame"
    assert W.widest_count(family, K, 1) == W.widest_count(family, K)
