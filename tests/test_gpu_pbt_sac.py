"""GPU tests of the population-based training scheduler's SAC kind (adc_engine_pbt_init_sac, then adc_engine_pbt_*; the kernels
k_pbt_exploit, k_pbt_exploit_ring and the new k_pbt_exploit_cell of parts/kernel_pbt.inc) over a SAC learner population: the batched
exploit against adc_engine_sac_pop_copy pair by pair, a whole round against a twin engine driven by hand with the primitives
and the numpy restatements tests/pbt_ref.py / tests/pbt_sac_ref.py, the temperature search with alpha_lr 0, resumption, refusals
and the Python scheduler.  Byte equality everywhere, no tolerance.  N = 12, K = 5, M = 6 (n = 2), T = 6 across an auto-reset,
policy hidden (20, 9) two-headed under the tight clamp, critics (11, 7, 1), batch 7, capacity 37: nothing is a multiple of 4 or of
a block, so the members' ring arrays start off 16-byte boundaries.  Neither the entry point nor the kind "sac" exists before this
feature: every test here fails on the parent commit."""
import ctypes as C
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
from tests import pbt_ref as B
from tests import pbt_sac_ref as BS
from tests import sac_ref as S
from tests import td3_ref as T3

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


@pytest.fixture(autouse=True)
def time_limit(request):
    """every test under its own time limit.  The alarm's handler runs when the interpreter next regains control: it ends a test
    that loops or waits in Python; a call that hangs inside the library is for the runner's outer limit to end."""
    seconds = 120

    def expired(*_):
        raise TimeoutError(f"{request.node.name} ran longer than {seconds} s")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(seconds)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


SEED = 41
RESETS = dict(max_days=4, auto_reset=True)
N, K, M, T = 12, 5, 6, 6
D, A = 5 * K + 2, K + 1
HIDDEN, WIDTHS, B0, CAPACITY = (20, 9), (11, 7, 1), 7, 37
CLAMP = (-1.0, -0.5)
ALPHA_LR_0, CLIPS, OWN_SEED = 3, 2, 1          # the member that keeps its temperature, the one that clips, the one with its own seed


def _options(**shared):
    """all different; five updates at target_update_interval 2 cross the Polyak gate both ways"""
    return [S.options(K, **dict(dict(critic_widths=WIDTHS, batch_size=B0, capacity=CAPACITY, target_update_interval=2, gamma=float(F(0.9 + 0.01 * m)),
                                     tau=float(F(0.01 * (m + 1))), actor_lr=float(F(1e-3 * (m + 1))), critic_lr=float(F(3e-3 / (m + 1))),
                                     alpha_lr=0.0 if m == ALPHA_LR_0 else float(F(1e-3 * (m + 1))), target_entropy=float(F(-1.0 - m)),
                                     init_alpha=float(F(0.3 + 0.2 * m)), reward_scale=0.5, seed=77 if m == OWN_SEED else 0,
                                     max_grad_norm=0.5 if m == CLIPS else 0.0), **shared)) for m in range(M)]


def _bounds():
    """budget in [50, 1500], bids in [0.02, 3 + k / 10]: shared by all members"""
    return np.concatenate([[50.0], np.full(K, 0.02)]).astype(F), np.concatenate([[1500.0], 3.0 + np.arange(K) / 10.0]).astype(F)


def _engine(amd):
    planes = H.implicit_params(N, K, SEED + 1, mean_volume=24, cvr=0.5)
    e = amd.StepEngine(N, K, seed=SEED, **RESETS)
    e.set_all_params(planes)
    e.reset()
    return e


def _members(seed=801):
    """per member a two-headed policy under the tight clamp (its log-std head's biases on both sides of it) and two critics"""
    rng = np.random.default_rng(seed)
    pols, crits = [], []
    for m in range(M):
        pol = S.sac_policy(rng, K, HIDDEN, "tanh", clamp=CLAMP, normalize=True, scale=0.6)
        pol.shift, pol.scale = R.realistic_norm(K)
        pol.layers[-1][1][A:] = np.linspace(CLAMP[0] - 0.6, CLAMP[1] + 0.6, A).astype(F)
        pols.append(pol)
        crits.append(T3.random_critics_for_tests(rng, K, WIDTHS))
    return pols, crits


def _install(e, pols, crits, opts):
    """learners, their squash, the record and the SAC population onto an engine that has a policy"""
    e.mlp_learners(M)
    for m in range(1, M):
        e.mlp_set_learner(m, pols[m])
    e.mlp_learners_set_squash(*_bounds())
    e.rollout_enable(T, obs=True)
    e.sac_pop_init(opts)
    for m in range(M):
        e.sac_pop_set_critics(m, crits[m])


def _population(amd, opts=None, seed=801):
    pols, crits = _members(seed)
    e = _engine(amd)
    e.mlp_init(pols[0], deterministic=False)
    _install(e, pols, crits, _options() if opts is None else opts)
    return e


def _iteration(e, updates=2):
    e.rollout_reset()
    e.run_days("mlp", T)
    e.sac_pop_store()
    return e.sac_pop_update(updates)


def _warm(*engines):
    """two iterations of collect, store and two updates: moments, cells and target critics are no longer their initial values"""
    for _ in range(2):
        stats = [_iteration(e) for e in engines]
    for s in stats[1:]:
        _assert_stats(stats[0], s, "the twins before anything")
    return stats[0]


def _snapshot(e):
    return [dict(e.sac_pop_state(m), params=e.mlp_learner_params(m), ring=e.sac_pop_buffer(m)) for m in range(M)]


def _assert_ring(a, b, what=""):
    for k in ("x", "a", "r", "done", "x2"):
        assert _same(a[k], b[k]), (k, what)
    assert (a["size"], a["written"], a["capacity"]) == (b["size"], b["written"], b["capacity"]), what


def _assert_member(x, y, what="", ring=True):
    for k in S.STATE_KEYS:                 # (log_alpha [3] among them: the cell's log_alpha, m, v)
        assert _same(x[k], y[k]), (k, what, x[k][:4], y[k][:4])
    assert x["updates"] == y["updates"], what
    assert _same(x["params"], y["params"]), ("the learner's stores", what)
    if ring:
        _assert_ring(x["ring"], y["ring"], what)


def _assert_equal(a, b, what=""):
    for m, (x, y) in enumerate(zip(a, b)):
        _assert_member(x, y, (m, what))


def _assert_stats(a, b, what=""):
    for m, (x, y) in enumerate(zip(a, b)):
        for k in S.STAT_KEYS + ("updates", "buffer_size"):
            assert _same(np.float64(x[k]), np.float64(y[k])), (k, m, x[k], y[k], what)


# ---- 1. the batched exploit equals the primitive pair by pair, without and with the ring ------------------------------------------
@pytest.mark.parametrize("with_ring", [False, True])
def test_batched_exploit_equals_pair_by_pair_copies(amd, with_ring):
    e1, e2 = _population(amd), _population(amd)
    e1.pbt_init("sac", replace_count=1, with_ring=with_ring)
    _warm(e1, e2)
    before = _snapshot(e1)
    assert before[0]["ring"]["size"] == 2 * T * (N // M) and not _same(before[1]["ring"]["x"], before[4]["ring"]["x"])
    assert before[0]["v_psi"].any() and not _same(before[0]["psi"], before[0]["psi_target"]) and before[0]["log_alpha"][1] != 0
    assert len({x["log_alpha"].tobytes() for x in before}) == M, "every member's cell is its own"
    e1.pbt_exploit([-1, 1, 2, -1, 4, -1])
    _assert_equal(_snapshot(e1), before, "keep all")
    pairs = ((4, 1), (4, 3), (5, 0))            # one donor feeds two destinations
    e1.pbt_exploit([5, 4, 2, 4, -1, -1])
    for src, dst in pairs:
        e2.sac_pop_copy(src, dst, with_ring=with_ring)
    after = _snapshot(e1)
    _assert_equal(after, _snapshot(e2), "after the copies")
    P = before[0]["theta"].size
    for src, dst in pairs:
        for k in S.STATE_KEYS:
            assert _same(after[dst][k], before[src][k]), (k, src, dst)
        assert _same(after[dst]["params"][:P], before[src]["theta"]), "the destination's policy layers were rebuilt from its theta"
        if with_ring:
            _assert_ring(after[dst]["ring"], before[src]["ring"], "the donor's ring came along")
        else:
            _assert_ring(after[dst]["ring"], before[dst]["ring"], "without the ring the destination keeps its own")
    for m in (2, 4, 5):
        _assert_member(after[m], before[m], ("untouched", m))
    assert e1.pbt_state()["round"] == 0, "the copy alone is no round"
    # the next act reads the rebuilt policy stores, the next update the rebuilt critic stores and the cell's fourth float
    # (member 3 keeps its temperature: its alpha statistic is the copied cell's alpha itself)
    s1, s2 = _iteration(e1, 1), _iteration(e2, 1)
    _assert_stats(s1, s2, "a further iteration")
    assert _same(F(s1[ALPHA_LR_0]["alpha"]), S.alpha_of(before[4]["log_alpha"][0])) and _same(F(s1[ALPHA_LR_0]["log_alpha"]), before[4]["log_alpha"][0])
    _assert_equal(_snapshot(e1), _snapshot(e2), "a further iteration")
    e1.close()
    e2.close()


# ---- 2. a whole round against a twin driven by hand -------------------------------------------------------------------------------
SAC_PBT = dict(replace_count=2, tuned=("actor_lr", "alpha_lr", "tau", "alpha", "target_entropy"), with_ring=True, fitness_ema=0.25, factors=(0.5, 2.0),
               bounds={"actor_lr": (1.5e-3, 5e-3), "alpha_lr": (0.0, 4e-3), "tau": (0.015, 0.05), "alpha": (0.4, 1.0), "target_entropy": (-7.0, -1.5)})


def _assert_result(res, ref, what=""):
    for k in ("fitness", "smoothed", "rank", "src", "hp"):
        assert _same(res[k], ref[k]), (k, res[k], ref[k], what)


def _by_hand(e, cfg, ref, opts):
    """the round `ref` (the restatement's result) on a twin through the primitives: copy, set_config and a state get / set that
    writes the restated log_alpha.  Returns what clamped: a set of (id, "lo" | "hi")"""
    clamped = set()
    cells = [e.sac_pop_state(m)["log_alpha"] for m in range(M)]
    old = BS.hp_of(opts)
    for m in range(M):
        src = int(ref["src"][m])
        if src < 0:
            continue
        e.sac_pop_copy(src, m, with_ring=bool(cfg["with_ring"]))
        opts[m] = dict(opts[m], **{BS.SAC_IDS[h]: float(ref["hp"][m, h]) for h in BS.HOST_IDS})
        e.sac_pop_set_config(m, **opts[m])
        la3, _ = BS.cell_after(cfg, ref["bits"][m], cells[src])
        st = e.sac_pop_state(m)
        assert _same(st["log_alpha"], cells[src]), "the primitive copies the cell verbatim"
        st["log_alpha"] = la3
        e.sac_pop_state(m, st)
        # what clamped, from the restatement's own arithmetic
        for h in range(len(BS.SAC_IDS)):
            if not (int(cfg["tuned_mask"]) >> h) & 1:
                continue
            up = (int(ref["bits"][m]) >> h) & 1
            if h == BS.ALPHA:
                raw = F(cells[src][0] + BS.shift_of(cfg, ref["bits"][m]))
                got = la3[0]
            else:
                raw = F(old[src, h] * F(cfg["factor_hi"] if up else cfg["factor_lo"]))
                got = ref["hp"][m, h]
            assert _same(got, B.clamp(raw, cfg["lo"][h], cfg["hi"][h]))
            if raw < cfg["lo"][h]:
                clamped.add((h, "lo"))
            if raw > cfg["hi"][h]:
                clamped.add((h, "hi"))
    return clamped


def test_whole_round_against_a_twin_driven_by_hand(amd):
    e1, e2 = _population(amd), _population(amd)
    e1.pbt_init("sac", **SAC_PBT)
    cfg = B.config_dict(amd.StepEngine.pbt_config("sac", M, **SAC_PBT))
    opts = _options()
    state, hp = dict(round=0, smoothed=np.zeros(M)), BS.hp_of(opts)
    nan_and_tie = np.array([2.0e6, 2.0e6, np.nan, -1.0e6, 5.0e6, 2.0e6])
    clamped = set()
    for rnd, handed in enumerate((None, nan_and_tie)):
        if rnd == 0:
            _warm(e1, e2)
        else:
            _assert_stats(_iteration(e1), _iteration(e2), "the iteration between the rounds")
        fit = e1.pbt_fitness() if handed is None else handed
        if handed is None:
            assert _same(fit, B.fitness(e1.rollout_fetch()["reward"], M))
        res = e1.pbt_step(handed)
        state, ref = BS.round_(cfg, SEED, state, fit, hp)
        _assert_result(res, ref, rnd)
        assert e1.pbt_state()["round"] == rnd + 1 and _same(e1.pbt_state()["smoothed"], state["smoothed"])
        replaced = [m for m in range(M) if res["src"][m] >= 0]
        assert len(replaced) == 2 and not set(replaced) & {int(res["src"][m]) for m in replaced}
        if handed is not None:
            assert res["rank"][2] == 0 and res["src"][2] >= 0, "the NaN ranks below every number and is replaced"
        hp = ref["hp"]
        clamped |= _by_hand(e2, cfg, ref, opts)
        _assert_equal(_snapshot(e1), _snapshot(e2), ("after the round", rnd))
        for m in replaced:
            assert _same(res["hp"][m, BS.ALPHA], BS.shift_of(cfg, ref["bits"][m])) and res["hp"][m, BS.ALPHA] != 0
        assert all(res["hp"][m, BS.ALPHA] == 0 for m in range(M) if m not in replaced)
    # under this seed: actor_lr, alpha_lr and tau clamp at hi, target_entropy at lo, log_alpha at hi (the bounds were chosen for it)
    assert any(side == "lo" for h, side in clamped if h != BS.ALPHA), ("a value was meant to clamp at lo", clamped)
    assert any(side == "hi" for h, side in clamped if h != BS.ALPHA), ("a value was meant to clamp at hi", clamped)
    assert any(h == BS.ALPHA for h, _ in clamped), ("the alpha clamp was meant to fire", clamped)
    _assert_stats(_iteration(e1), _iteration(e2), "the iteration after the rounds")
    _assert_equal(_snapshot(e1), _snapshot(e2), "the iteration after the rounds")
    e1.close()
    e2.close()


# ---- 3. the temperature search: alpha_lr 0 in every member ------------------------------------------------------------------------
def test_temperature_search_with_alpha_lr_0(amd):
    opts = _options(alpha_lr=0.0)
    e = _population(amd, opts)
    options = dict(replace_count=3, tuned=("alpha",), bounds={"alpha": (0.6, 2.0)}, factors=(0.5, 2.0))
    e.pbt_init("sac", **options)
    cfg = B.config_dict(amd.StepEngine.pbt_config("sac", M, **options))
    _warm(e)
    cells = [e.sac_pop_state(m)["log_alpha"] for m in range(M)]
    for m in range(M):
        assert _same(cells[m], np.array([S.log_alpha_init(opts[m]["init_alpha"]), 0, 0], F)), "no temperature step ever ran"
    fit = np.arange(M, dtype=np.float64)
    res = e.pbt_step(fit)
    _, ref = BS.round_(cfg, SEED, dict(round=0, smoothed=np.zeros(M)), fit, BS.hp_of(opts))
    _assert_result(res, ref)
    assert [m for m in range(M) if res["src"][m] >= 0] == [0, 1, 2]
    expected = []
    for m in range(M):
        src = int(res["src"][m])
        la3 = cells[m] if src < 0 else BS.cell_after(cfg, ref["bits"][m], cells[src])[0]
        expected.append(la3)
        got = e.sac_pop_state(m)["log_alpha"]
        assert _same(got, la3), (m, got, la3)
        if src >= 0:
            assert not _same(got, cells[m]) and not _same(got, cells[src]), "the cell moved although alpha_lr is 0"
            assert cfg["lo"][4] <= got[0] <= cfg["hi"][4]
            assert _same(got[0], B.clamp(F(cells[src][0] + res["hp"][m, 4]), cfg["lo"][4], cfg["hi"][4]))
        assert _same(e.sac_pop_state(m)["log_alpha"][1:], np.zeros(2, F))
    # init_alpha 0.9 .. 1.3 in the donors, halved or doubled, against [0.6, 2]: under this seed a shift is cut by a bound, another is not
    cut = [_same(expected[m][0], cfg["lo"][4]) or _same(expected[m][0], cfg["hi"][4]) for m in (0, 1, 2)]
    assert any(cut) and not all(cut), cut
    stats = _iteration(e, 1)
    for m in range(M):
        assert _same(F(stats[m]["alpha"]), S.alpha_of(expected[m][0])) and _same(F(stats[m]["log_alpha"]), expected[m][0]), m
        assert _same(e.sac_pop_state(m)["log_alpha"], expected[m]), "alpha_lr 0: the update leaves the cell"
    e.close()


# ---- 4. resume --------------------------------------------------------------------------------------------------------------------
def test_a_resumed_run_continues_bit_for_bit(amd):
    e1, e2 = _population(amd), _population(amd)
    e1.pbt_init("sac", **SAC_PBT)
    _warm(e1, e2)
    first = e1.pbt_step()
    assert not _same(e1.sac_pop_state(int(np.argmax(first["src"] >= 0)))["theta"], e2.sac_pop_state(int(np.argmax(first["src"] >= 0)))["theta"])
    # the fresh engine has seen the same days; it is handed every member's state, ring and configuration and the scheduler's state
    opts = _options()
    for m in range(M):
        e2.sac_pop_state(m, e1.sac_pop_state(m))
        e2.sac_pop_buffer_load(m, e1.sac_pop_buffer(m))
        e2.sac_pop_set_config(m, **dict(opts[m], **{BS.SAC_IDS[h]: float(first["hp"][m, h]) for h in BS.HOST_IDS}))
    from adcraft_amd import _ffi
    with pytest.raises(_ffi.EngineStateError):
        e2.pbt_state()
    e2.pbt_init("sac", **SAC_PBT)
    saved = e1.pbt_state()
    assert saved["round"] == 1
    e2.pbt_state(saved)
    assert e2.pbt_state()["round"] == 1 and _same(e2.pbt_state()["smoothed"], saved["smoothed"])
    _assert_equal(_snapshot(e1), _snapshot(e2), "restored")
    for rnd in range(2):
        _assert_stats(_iteration(e1), _iteration(e2), rnd)
        r1, r2 = e1.pbt_step(), e2.pbt_step()
        _assert_result(r1, r2, rnd)
        _assert_equal(_snapshot(e1), _snapshot(e2), rnd)
    assert e1.pbt_state()["round"] == 3
    _assert_stats(_iteration(e1), _iteration(e2), "after the rounds")
    e1.close()
    e2.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(amd):
    from adcraft_amd import _ffi
    pols, crits = _members()
    # no trainer; a solo SAC trainer; a TD3 population
    e = _engine(amd)
    with pytest.raises(_ffi.EngineStateError, match="SAC population"):
        e.pbt_init("sac", replace_count=1)
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_set_squash(*_bounds())
    e.rollout_enable(T, obs=True)
    e.sac_init(**_options()[0])
    with pytest.raises(_ffi.EngineStateError, match="SAC population"):
        e.pbt_init("sac", replace_count=1)
    e.close()
    e = _engine(amd)
    rng = np.random.default_rng(5)
    plain = R.random_policy(rng, K, HIDDEN, "tanh", normalize=True, scale=0.6)
    plain.shift, plain.scale = R.realistic_norm(K)
    plain.log_std = np.zeros(A, F)
    e.mlp_init(plain, deterministic=False)
    e.mlp_learners(M)
    e.rollout_enable(T, obs=True)
    e.td3_pop_init([T3.options(critic_widths=WIDTHS, batch_size=B0, capacity=CAPACITY)])
    with pytest.raises(_ffi.EngineStateError, match="SAC population"):
        e.pbt_init("sac", replace_count=1)
    e.pbt_init("td3", replace_count=1)           # the engine is usable, and the TD3 kind is what it was
    assert e.pbt_state()["round"] == 0
    e.close()
    # q out of range (through the C entry point: Python's own check would refuse first)
    e = _population(amd)
    cfg = amd.StepEngine.pbt_config("sac", M, 1)
    for q in (0, M // 2 + 1):
        cfg.replace_count = q
        assert e._lib.adc_engine_pbt_init_sac(e._h, C.byref(cfg)) == _ffi.ADC_EINVAL
    with pytest.raises(ValueError, match="replace_count"):
        e.pbt_init("sac", replace_count=M // 2 + 1)
    with pytest.raises(ValueError, match="tuned_mask|not a tunable"):
        e.pbt_init("sac", replace_count=1, tuned=("sigma",), bounds={"sigma": (0.1, 1.0)})
    with pytest.raises(_ffi.EngineStateError):
        e.pbt_fitness()
    e.pbt_init("sac", replace_count=3)
    # no day recorded
    with pytest.raises(_ffi.EngineStateError, match="no recorded day"):
        e.pbt_fitness()
    with pytest.raises(_ffi.EngineStateError, match="no recorded day"):
        e.pbt_step()
    _iteration(e)
    before = _snapshot(e)
    # a destination that is a source; a member that does not exist
    with pytest.raises(ValueError, match="also a source"):
        e.pbt_exploit([1, 2, -1, -1, -1, -1])
    with pytest.raises(ValueError, match="src_of_m"):
        e.pbt_exploit([M, -1, -1, -1, -1, -1])
    with pytest.raises(ValueError):
        e.pbt_exploit([-1] * (M - 1))
    with pytest.raises(ValueError):
        e.pbt_step(np.zeros(M + 1))
    _assert_equal(_snapshot(e), before, "a refused call changes nothing")
    assert e.pbt_state()["round"] == 0
    res = e.pbt_step()
    assert (res["src"] >= 0).sum() == 3 and e.pbt_state()["round"] == 1
    _iteration(e)

    def gone():
        for call in (e.pbt_step, e.pbt_fitness, e.pbt_state, lambda: e.pbt_exploit([-1] * M)):
            with pytest.raises(_ffi.EngineStateError, match="adc_engine_pbt_init"):
                call()

    def again(q):
        e.pbt_init("sac", replace_count=q)
        assert e.pbt_state()["round"] == 0 and not e.pbt_state()["smoothed"].any(), "a new scheduler starts at round 0"
        _iteration(e)
        assert (e.pbt_step()["src"] >= 0).sum() == q and e.pbt_state()["round"] == 1

    # the scheduler goes with the learners (and the trainer over them) ...
    e.mlp_learners(M)
    gone()
    with pytest.raises(_ffi.EngineStateError, match="SAC population"):
        e.pbt_init("sac", replace_count=1)
    _install(e, pols, crits, _options())
    gone()
    again(1)
    # ... with the record ...
    e.rollout_enable(T, obs=True)
    gone()
    e.sac_pop_init(_options())
    for m in range(M):
        e.sac_pop_set_critics(m, crits[m])
    again(2)
    # ... and with a new population over the old one
    e.sac_pop_init(_options())
    gone()
    for m in range(M):
        e.sac_pop_set_critics(m, crits[m])
    again(3)
    e.close()


# ---- 6. the Python scheduler over the SAC population trainer ----------------------------------------------------------------------
def test_scheduler_over_the_sac_population_trainer(amd):
    from adcraft_amd.baselines.pbt import PBTScheduler
    from adcraft_amd.baselines.sac_trainer import SACPopulationTrainer
    pols, crits = _members()
    keys = ("gamma", "tau", "actor_lr", "critic_lr", "alpha_lr", "target_entropy", "init_alpha", "reward_scale", "seed", "max_grad_norm")
    configs = [dict({k: o[k] for k in keys}, critic_hidden=WIDTHS[:-1], batch_size=B0, capacity=CAPACITY, target_update_interval=2, learning_starts=0,
                    updates_per_iteration=2, critics=crits[m]) for m, o in enumerate(_options())]
    e = _engine(amd)
    tr = SACPopulationTrainer(e, pols, configs, *_bounds(), horizon=T)
    bounds = {"actor_lr": (1.5e-3, 5e-3), "alpha": (0.4, 1.0), "target_entropy": (-7.0, -1.5)}
    sch = PBTScheduler(tr, replace_fraction=0.34, tuned=("actor_lr", "alpha", "target_entropy"), bounds=bounds, factors=(0.5, 2.0), every=2, seed=9,
                       with_ring=True)
    assert sch.kind == "sac" and sch.replace_count == 2
    start = [dict(c) for c in tr.configs]
    tr.iteration()
    assert sch.step() is None and e.pbt_state()["round"] == 0
    tr.iteration()
    cells = [e.sac_pop_state(m)["log_alpha"] for m in range(M)]
    res = sch.step()
    assert res is not None and e.pbt_state()["round"] == 1 and len(sch.history) == 1 and res["origin"] == sch.origin
    assert (res["src"] >= 0).sum() == 2
    for m in range(M):
        src = int(res["src"][m])
        for h, name in enumerate(sch.ids):
            if name == "alpha":
                continue
            assert _same(F(tr.configs[m][name]), res["hp"][m, h]), (m, name)
        assert tr.configs[m]["init_alpha"] == start[m]["init_alpha"], "the temperature has no host mirror: init_alpha is left alone"
        if src < 0:
            assert tr.configs[m] == start[m] and sch.origin[m] == m
            assert _same(e.sac_pop_state(m)["log_alpha"], cells[m])
        else:
            assert sch.origin[m] == src
            for name in ("actor_lr", "target_entropy"):
                lo, hi = bounds[name]
                assert tr.configs[m][name] in (float(np.clip(F(F(start[src][name]) * F(f)), F(lo), F(hi))) for f in (0.5, 2.0)), (m, name)
            for name in ("critic_lr", "alpha_lr", "tau", "gamma", "seed", "max_grad_norm"):
                assert tr.configs[m][name] == start[m][name], "untuned fields stay the member's own"
            la = e.sac_pop_state(m)["log_alpha"]
            assert _same(la[0], B.clamp(F(cells[src][0] + res["hp"][m, 4]), F(np.log(0.4)), F(np.log(1.0)))) and _same(la[1:], cells[src][1:])
            _assert_ring(e.sac_pop_buffer(m), e.sac_pop_buffer(src), "the donor's ring came along")
    # the engine's table is what the dicts say: writing the dicts again changes nothing in the next update
    twin_pols, _ = _members()
    e2 = _engine(amd)
    tr2 = SACPopulationTrainer(e2, twin_pols, configs, *_bounds(), horizon=T)
    tr2.iteration()
    tr2.iteration()
    e2.pbt_init("sac", replace_count=2, with_ring=True)
    e2.pbt_exploit([int(s) for s in res["src"]])
    for m in range(M):
        if res["src"][m] >= 0:
            st = e2.sac_pop_state(m)
            st["log_alpha"] = e.sac_pop_state(m)["log_alpha"]
            e2.sac_pop_state(m, st)
        tr2.set_config(m, **{k: v for k, v in tr.configs[m].items() if k in keys})
    s1, s2 = tr.iteration(), tr2.iteration()
    assert len(s1) == M
    _assert_stats(s1, s2, "the dicts drive a twin to the same bits")
    with pytest.raises(TypeError):
        PBTScheduler(object())
    e.close()
    e2.close()
