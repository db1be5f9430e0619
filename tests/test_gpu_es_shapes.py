"""GPU tests of the evolution strategy's kernels (parts/kernel_es.inc) at the shapes where their launch shape and their loops take
another path, bit for bit against the numpy restatement tests/es_ref.py, the host twins adc_es_noise_host /
adc_es_update_host where the restatement's per-quad loop would be too slow, and the act's host twins on the perturbed weights.

k_es_update: a workgroup owns 16 quads (64 parameters); sixteen lanes a quad leave the products of sixteen pairs a round in
prod[16][64], one lane a parameter adds n of those rows between two barriers; more than 16 pairs (M > 32) take more than one round
and a pair count that is no multiple of 16 ends on a partial one, the rows of the round before still in prod.  k_es_perturb: a
workgroup owns 256 quads (1024 parameters), the Philox counter is q = blockIdx.x * 256 + threadIdx.x.  param_locate writes a
member's chain-major slots and reads them back: only an act on the written weights tells whether the slots are the right ones.
k_es_accumulate: a workgroup owns 256 envs, an env group starts where its first env is."""
import numpy as np
import pytest

from tests import es_ref as E
from tests import gru_ref as G
from tests import helpers as H
from tests import learner_shapes as LS
from tests import mlp_ref as R
from tests.test_gpu_recurrent import Twin, _assert_hidden, _assert_last

pytestmark = pytest.mark.gpu
F = np.float32
BUDGET = 1000.0                                                        # (Twin's: tests/test_gpu_recurrent.py acts under it)
FOREVER = dict(max_days=1 << 20, loss_threshold=1e12)


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _engine(amd, N, K, seed=3, **kw):
    e = amd.StepEngine(N, K, seed=seed, **kw)
    e.set_all_params(H.implicit_params(N, K, seed + 1, mean_volume=24, cvr=0.5))
    e.reset()
    return e


def _assert_state(e, ref, what):
    """theta, m, v of the strategy and the centre's chain-major copy against ref = (theta, m, v, ...)"""
    st = e.es_state()
    for k, want in zip(("theta", "m", "v"), ref):
        assert _same(st[k], want), (what, k, int(np.sum(st[k].view(np.uint32) != want.view(np.uint32))))
    assert _same(e.mlp_params(), ref[0]), (what, "the centre")


def _assert_telling(fit, shaping, rows, g, what):
    """on the reference alone: the case can tell a sum cut after its first round, a round that adds rows it did not write, and a
    lost term from the law - every pair has a term, the first sixteen pairs' float64 sum is the whole sum in no parameter, no
    entry of the gradient is zero"""
    u = E.shape(fit, shaping)
    du = u[0::2] - u[1::2]
    assert np.all(du != 0) and np.all(np.isfinite(du)), (what, du)
    if shaping == "raw":
        assert len(set(du.tolist())) == du.size, (what, "two pairs share a du")
    acc = np.zeros(rows.shape[1], np.float64)
    for i in range(du.size):
        if i == 16:
            first = acc.copy()
        acc = acc + du[i] * rows[i].astype(np.float64)
    if du.size > 16:
        assert np.all(first != acc), (what, "the rounds after the first change nothing somewhere")
    assert np.all(g != 0), what


# ---- a. pairs across rounds -------------------------------------------------------------------------------------------------------------
# (Adam under centred ranks, with ties and NaNs in the second generation; SGD under raw fitness - every pair its own du - with an
# L2 decay.  seed 0: the engine's)
ES_KW = [dict(sigma=0.05, lr=0.02, seed=99), dict(sigma=0.02, lr=0.05, optimiser="sgd", shaping="raw", l2=0.001, seed=0)]
ROUNDS_K, ROUNDS_HIDDEN, ROUNDS_P = 10, (8,), 523


@pytest.mark.parametrize("case", range(len(ES_KW)), ids=["adam-ranks", "sgd-raw-l2"])
@pytest.mark.parametrize("M", [30, 32, 34, 66, 512])
def test_two_generations_over_partial_exact_and_many_rounds(amd, M, case):
    """K = 10, hidden (8,): P = 523 = 4 * 130 + 3 = 8 * 64 + 11 - the last quad holds three parameters, the ninth update workgroup
    eleven.  One env a member.  M / 2 = 15 (one partial round), 16 (one exact round), 17 and 33 (full rounds and one pair: fifteen
    rows of the round before stay in prod), 256 (sixteen rounds, the shape the kernel's comment measured).  Two generations from
    fitness handed in, so that the moments and the generation word are not zero in the second: every member after the
    perturbation (M = 512: the first pair, the last pair and 16 others), then theta, m, v and the centre after the update, are the
    restatement's.  (Under raw shaping the second generation's ties lie across pairs: a tie inside a pair is a pair with du = 0,
    which the case must not have.)"""
    kw = dict(ES_KW[case])
    K, P = ROUNDS_K, ROUNDS_P
    rng = np.random.default_rng(1000 * case + M)
    pol = R.random_policy(rng, K, ROUNDS_HIDDEN, "tanh", scale=0.3)
    e = _engine(amd, M, K, seed=61)
    e.mlp_init(pol, rng.integers(0, 2 ** 63, M).astype(np.uint64))
    e.mlp_population(M)
    e.es_init(**kw)
    assert e.mlp_param_count() == P == (5 * K + 2 + 1) * 8 + (8 + 1) * (K + 1) and P % 4 == 3 and P % 64 == 11
    noise_seed = kw["seed"] or 61
    law = {k: v for k, v in kw.items() if k != "seed"}
    shaping = law.get("shaping", "centered_rank")
    ranks = shaping == "centered_rank"
    sample = range(M) if M < 512 else sorted({0, 1, M - 2, M - 1} | set(rng.choice(np.arange(2, M - 2), 16, replace=False).tolist()))
    ref = (E.flat_params(pol), np.zeros(P, F), np.zeros(P, F))
    for g in range(2):
        rows = E.noise_rows(noise_seed, g, M // 2, P)
        e.es_perturb()
        ref_members = E.members(ref[0], noise_seed, g, M, kw["sigma"], rows=rows)
        for mem in sample:
            assert _same(e.mlp_member_params(mem), ref_members[mem]), (g, mem)
        fit = E.draw_fitness(rng, M, ties=g == 1, nans=ranks and g == 1, tie_in_pair=ranks)
        new = E.update(*ref, fit, noise_seed, g, rows=rows, **law)
        _assert_telling(fit, shaping, rows, new[3], (M, case, g))
        stats = e.es_update(fit)
        _assert_state(e, new, (M, case, g))
        assert stats["generation"] == g + 1 == e.es_state()["generation"]
        assert abs(stats["grad_norm"] - np.linalg.norm(new[3].astype(np.float64))) < 1e-9 * (1 + stats["grad_norm"])
        assert not _same(new[0], ref[0])
        ref = new[:3]
    assert ranks == bool(ref[1].any()), "Adam's moments moved; SGD has none"
    e.close()


# ---- b. wide, ragged and deep flat vectors ----------------------------------------------------------------------------------------------
GENERATION, WIDE_M = 300, 34
# the strategy per shape; P from the widths; the workgroups of k_es_perturb and k_es_update
WIDE = dict(W1=(dict(sigma=0.05, lr=0.02, l2=0.001, seed=99), 127345, 125, 1990),
            W2=(dict(sigma=0.02, lr=0.0001, optimiser="sgd", shaping="raw", l2=0.001, seed=0), 63143, 62, 987),
            W3=(dict(sigma=0.03, lr=0.01, shaping="raw", beta1=0.8, beta2=0.99, seed=7), 56221, 55, 879))


def _terms(widths):
    """(begin, first bias, end) in the flat order of every term (n_in, n_out)"""
    out, pos = [], 0
    for n_in, n_out in widths:
        out.append((pos, pos + n_in * n_out, pos + (n_in + 1) * n_out))
        pos = out[-1][2]
    return out


def _ranges(terms, P):
    """the ranges the restatement is run on: the first and the last 64 parameters, 32 on either side of every term's begin and of
    every term's first bias"""
    edges = sorted({t[0] for t in terms[1:]} | {t[1] for t in terms})
    return [(0, 64), (P - 64, P)] + [(max(0, x - 32), min(P, x + 32)) for x in edges]


def _wide_policy(rng, name):
    K = LS.SHAPES[name]["K"]
    pol = (LS.td3_policy if name == "W1" else LS.pg_policy)(rng, name, normalize=True)
    pol.shift, pol.scale = R.realistic_norm(K)
    pol.layers[-1][1][1:K + 1] += F(0.3)                               # bids around 80 cents: auctions are won
    widths = [w.shape for w, _ in pol.layers]
    return pol, widths


def _act_all(e, lib, pols, keys, obs, tick, what):
    """the engine's last act and the actions it left for the env, against the feed-forward act's host twin env by env"""
    st = e.mlp_last()
    st["bids"], st["budget"] = e.get_actions()
    assert _same(e.mlp_agent_state()[1], np.full(e.num_envs, tick + 1, np.uint32)), what
    for env in range(e.num_envs):
        ref = R.twin_act(lib, pols[env], None if obs is None else obs[env], key=keys[env], tick=tick, budget_override=BUDGET)
        for k in ("mean", "log_std", "action", "logp", "value", "bids", "budget"):
            assert _same(st[k][env], ref[k][0]), (what, env, k)
    return st


@pytest.mark.parametrize("name", ["W1", "W2", "W3"])
def test_wide_flat_vectors_perturbed_acted_on_and_updated(amd, lib, name):
    """the shapes of tests/learner_shapes.py under 34 members (17 pairs: two rounds of the update), one env each, from generation
    300 and moments that are not zero:
      W1  K = 40, hidden (256, 255, 33), 41 outputs: P = 127 345 = 1 mod 4, 125 workgroups of the perturbation, 1990 of the update
      W2  K = 130, hidden (33, 250, 64), two heads (262 outputs): P = 63 143 = 3 mod 4, four terms
      W3  K = 256, hidden (31,), two heads (514): P = 56 221 = 1 mod 4; n_in = 1282 is 40 blocks of 32 inputs and one of two
    Every member after the perturbation is theta + sigma * (+-noise twin) in full, and the restatement's on the first and last 64
    parameters and 32 either side of every term's begin and first bias.  Then the act, which alone reads the slots param_locate
    wrote: on day 0 (zeros, normalised) and on the observation that day left, every env's act - means, log-stds, action, log-probability, value, bids,
    budget - is the host twin's under policy_from_flat(centre, its member).  The update is the update twin's in full and the
    restatement's on the same ranges; the population turned off, the centre acts as policy_from_flat(centre, theta) does."""
    from adcraft_amd.baselines.es_trainer import policy_from_flat
    kw, P, perturb_groups, update_groups = WIDE[name]
    M = N = WIDE_M
    K = LS.SHAPES[name]["K"]
    rng = np.random.default_rng(sum(map(ord, name)))
    pol, widths = _wide_policy(rng, name)
    terms = _terms(widths)
    assert terms[-1][2] == P and (P % 4, len(terms)) == dict(W1=(1, 4), W2=(3, 4), W3=(1, 2))[name]
    assert ((P + 3) // 4 + 255) // 256 == perturb_groups and ((P + 3) // 4 + 15) // 16 == update_groups
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    keys = [R.agent_key(s) for s in seeds]
    e = _engine(amd, N, K, seed=61, **FOREVER)
    e.mlp_init(pol, seeds)
    assert e.mlp_param_count() == P
    e.mlp_population(M)
    e.es_init(**kw)
    noise_seed = kw["seed"] or 61
    law = {k: v for k, v in kw.items() if k != "seed"}
    theta = E.flat_params(pol)
    mom = ((rng.standard_normal(P) * 0.01).astype(F), (rng.random(P) * 1e-4).astype(F))
    e.es_state(dict(theta=theta, m=mom[0], v=mom[1], generation=GENERATION))
    ranges = _ranges(terms, P)
    # the perturbation
    e.es_perturb()
    sigma = F(kw["sigma"])
    got = np.stack([e.mlp_member_params(m) for m in range(M)])
    ref_members = np.zeros((M, P), F)
    for i in range(M // 2):
        eps = E.twin_noise(lib, noise_seed, i, GENERATION, 0, P)
        ref_members[2 * i], ref_members[2 * i + 1] = theta + sigma * eps, theta + sigma * (-eps)
    for m in range(M):
        assert _same(got[m], ref_members[m]), (name, m, int(np.sum(got[m] != ref_members[m])))
    rows = {}
    for a, b in ranges:
        rows[a] = E.noise_rows(noise_seed, GENERATION, M // 2, b, a)
        part = E.members(theta[a:b], noise_seed, GENERATION, M, kw["sigma"], rows=rows[a])
        assert _same(got[:, a:b], part), (name, a, b)
    assert _same(e.mlp_params(), theta)
    # the act on the written slots: day 0, then the observation it left
    pols = [policy_from_flat(pol, ref_members[m]) for m in range(M)]
    e.mlp_step(BUDGET)
    first = _act_all(e, lib, pols, keys, None, 0, (name, "day 0"))
    obs = R.flat_obs(e.fetch())
    assert np.abs(obs).sum() > 0
    e.mlp_act(BUDGET)
    second = _act_all(e, lib, pols, keys, obs, 1, (name, "day 1"))
    assert not _same(first["mean"], second["mean"]) and len({r.tobytes() for r in second["mean"]}) == N, "members differ, days differ"
    # the update
    fit = E.draw_fitness(rng, M, ties=True, nans=law.get("shaping") != "raw", tie_in_pair=law.get("shaping") != "raw")
    new = E.twin_update(lib, theta, *mom, fit, noise_seed, GENERATION, **law)
    stats = e.es_update(fit)
    _assert_state(e, new, name)
    assert stats["generation"] == GENERATION + 1
    assert abs(stats["grad_norm"] - np.linalg.norm(new[3].astype(np.float64))) < 1e-9 * (1 + stats["grad_norm"])
    st = e.es_state()
    for a, b in ranges:
        part = E.update(theta[a:b], mom[0][a:b], mom[1][a:b], fit, noise_seed, GENERATION, p0=a, rows=rows[a], **law)
        _assert_telling(fit, law.get("shaping", "centered_rank"), rows[a], part[3], (name, a, b))
        for k, want in zip(("theta", "m", "v"), part):
            assert _same(st[k][a:b], want), (name, a, b, k)
    assert np.all(new[0] != theta)
    # the centre follows theta: evaluation without a population sees it
    e.mlp_population(0)
    e.mlp_act(BUDGET)
    _act_all(e, lib, [policy_from_flat(pol, new[0])] * N, keys, obs, 2, (name, "the centre"))
    e.close()


def test_a_recurrent_policy_of_six_terms(amd, lib):
    """as many terms as the flat order holds (kMlpMaxTerms = 6): a trunk of three layers - the deepest mlp_init accepts - a cell's
    Wi | bi and Wh | bh, the output layer; K = 4, trunk (33, 7, 9), G = 5: P = 1339 = 3 mod 4, two workgroups of the perturbation.
    34 members, one env each, from generation 300: members and update against the restatement and the twin in full; the act on
    day 0 (from zeros) and on day 1 (from a state, through Wh) under every member's parameters, and the centre's on day 2 after the
    update, through tests/test_gpu_recurrent.py's Twin, the state h and its words too"""
    from adcraft_amd.baselines.es_trainer import flat_params, policy_from_flat
    K, trunk, width, M = 4, (33, 7, 9), 5, WIDE_M
    N = M
    kw = dict(sigma=0.05, lr=0.02, seed=99)
    rng = np.random.default_rng(66)
    pol = G.random_policy(rng, K, trunk, width, "tanh", value=True, normalize=True, scale=0.6)
    pol.shift, pol.scale = R.realistic_norm(K)
    D, A = 5 * K + 2, K + 1
    terms = _terms([(D, 33), (33, 7), (7, 9), (9, 3 * width), (width, 3 * width), (width, A)])
    P = terms[-1][2]
    assert len(terms) == 6 and P == 1339 and P % 4 == 3
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    e = _engine(amd, N, K, seed=47, **FOREVER)
    e.mlp_init(pol, seeds, deterministic=False)
    assert e.mlp_param_count() == P and e.mlp_gru_width() == width
    e.mlp_population(M)
    e.es_init(**kw)
    theta = flat_params(pol)
    mom = ((rng.standard_normal(P) * 0.01).astype(F), (rng.random(P) * 1e-4).astype(F))
    e.es_state(dict(theta=theta, m=mom[0], v=mom[1], generation=GENERATION))
    e.es_perturb()
    rows = E.noise_rows(kw["seed"], GENERATION, M // 2, P)
    ref_members = E.members(theta, kw["seed"], GENERATION, M, kw["sigma"], rows=rows)
    for m in range(M):
        assert _same(e.mlp_member_params(m), ref_members[m]), m
    twin = Twin(lib, e, seeds)
    pols = [policy_from_flat(pol, ref_members[m]) for m in range(M)]
    for day in range(2):
        ref = twin.act(pols)
        assert all(twin.zeros) == (day == 0)
        e.mlp_step(BUDGET)
        _assert_last(e, ref, ("members", day))
        _assert_hidden(e, twin, ("members", day))
    assert len({r.tobytes() for r in ref["mean"]}) == N
    fit = E.draw_fitness(rng, M, ties=True, nans=True)
    new = E.update(theta, *mom, fit, kw["seed"], GENERATION, sigma=kw["sigma"], lr=kw["lr"], rows=rows)
    tw = E.twin_update(lib, theta, *mom, fit, kw["seed"], GENERATION, sigma=kw["sigma"], lr=kw["lr"])
    assert all(_same(a, b) for a, b in zip(new, tw))
    _assert_telling(fit, "centered_rank", rows, new[3], "recurrent")
    e.es_update(fit)
    _assert_state(e, new, "recurrent")
    e.mlp_population(0)
    ref = twin.act(policy_from_flat(pol, new[0]))
    assert not any(twin.zeros)
    e.mlp_step(BUDGET)
    _assert_last(e, ref, "the centre")
    _assert_hidden(e, twin, "the centre")
    e.close()


# ---- c. fitness over more than one block of envs ------------------------------------------------------------------------------------------
def test_fitness_over_three_blocks_of_envs_and_uneven_members(amd):
    """N = 520: three workgroups of k_es_accumulate, the last of 8 envs; under four env groups of 130 no group's first env is a
    multiple of 256.  8 members over an uneven map: member 0 owns one env, member 1 owns 300 - more than a block - in two runs,
    the others what is left, interleaved.  Two days through run_days("mlp"): es_fitness() is E.fitness of the per-env float64
    sums of the step rewards, and the same bits under one env group and under four"""
    N, K, M, days = 520, 3, 8, 2
    member_of_env = np.zeros(N, np.int32)
    member_of_env[1:201] = 1
    member_of_env[201:420] = 2 + np.arange(219) % 6
    member_of_env[420:] = 1
    count = np.bincount(member_of_env, minlength=M)
    assert count[0] == 1 and count[1] == 300 and count.min() == 1 and count.sum() == N
    rng = np.random.default_rng(12)
    pol = R.random_policy(rng, K, (4,), "tanh", scale=0.3)
    pol.layers[-1][1][1:K + 1] += F(0.5)
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    fits = []
    for groups in (1, 4):
        e = _engine(amd, N, K, seed=71, max_days=4, auto_reset=True)
        e.set_env_groups(groups)
        e.mlp_init(pol, seeds)
        e.mlp_population(M, member_of_env)
        e.es_init(sigma=0.3, seed=5)
        e.es_perturb()
        ret = np.zeros(N, np.float64)
        for _ in range(days):
            e.run_days("mlp", 1, BUDGET)
            ret = ret + np.asarray(e.fetch()["reward"], np.float64)
        assert e.env_groups() == groups, "the env groups did not engage"
        fit = e.es_fitness()
        assert _same(fit, E.fitness(ret, member_of_env, M)), (groups, fit)
        assert len(set(fit.tolist())) == M and np.count_nonzero(ret) > N // 2, "members differ, envs earn"
        fits.append(fit)
        e.close()
    assert _same(fits[0], fits[1])
