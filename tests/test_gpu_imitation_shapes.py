"""GPU tests of the imitation kernel at wide, deep and ragged network shapes (the shapes W1-W3 of
tests/learner_shapes.py).  k_im_sample is pg_sample_body's imitation instance, compiled on its own: its own register allocation
over the policy-gradient trainer's hand-carved dynamic LDS.  The other imitation and DAgger tests run it at hidden (13, 8) and
K <= 10; here only the network varies: 8 envs, 5 teacher days under the fixed teacher, 40 samples.

1. the device against the numpy restatement tests/im_ref.py bit for bit at W1-W3: the returns through an auto-reset, two
   minibatch steps, the moving scale;
2. the device's gradient - read exactly from the first moment after one Adam step with beta1 = 0 - against PyTorch float64
   autograd of the imitation loss (tests/test_imitation_host.py::_torch_im_grad) under learner_shapes.yardstick;
3. the last K the trainer's LDS limit accepts, one imitation step bit for bit: the kernel's launch with the whole 64 KiB carve.
Measured figures: profiles/pr_imitation_shapes.txt."""
import signal

import numpy as np
import pytest

from tests import im_ref as I
from tests import learner_shapes as W
from tests import pg_ref as P
from tests.test_gpu_imitation import _assert_state, _assert_stats, _fresh_state, _same
from tests.test_gpu_learner_shapes import N, T, _engine, _normed
from tests.test_imitation_host import W_IM, Z_MAX, _torch_im_grad, conditioned, z64

pytestmark = pytest.mark.gpu
F = np.float32
NAMES = ("W1", "W2", "W3")
RESETS = dict(max_days=3, auto_reset=True)
# one seed a case: the policy's draw, the engine's streams and the agents'
IM_SEED = dict(W1=211, W2=213, W3=217)
_inputs = {}


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


@pytest.fixture(autouse=True)
def time_limit(request):
    """every test under its own time limit (the handler runs when the interpreter next regains control)"""
    seconds = 120

    def expired(*_):
        raise TimeoutError(f"{request.node.name} ran longer than {seconds} s")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(seconds)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _options(**kw):
    return P.options(lr=1e-3, gamma=0.9, reward_scale=0.05, **kw)


def _trainer(amd, pol, K, seed, opts, im, envs=N, days=T, **engine):
    """an engine under the fixed teacher (budget 40, bids in [0.3, 1]) with the imitation trainer alive over `pol`"""
    e = _engine(amd, K, seed, envs=envs, **engine)
    e.sample_actions(0.3, 1.0, 40.0)
    e.mlp_init(pol, np.random.default_rng(seed).integers(0, 2 ** 63, envs).astype(np.uint64), deterministic=False)
    e.rollout_enable(days, obs=True)
    e.pg_init(**opts)
    e.im_init(**im)
    return e


def _teacher_inputs(amd, name):
    """(input rows [T N, D], teacher actions [T N, A]) of the shape's teacher days, collected once: a teacher day's input row is the
    env's observation under the policy's shift / scale and its action the teacher's - neither depends on the learner's weights"""
    if name not in _inputs:
        K, seed = W.SHAPES[name]["K"], IM_SEED[name]
        pol = _normed(W.pg_policy(np.random.default_rng(seed), name, normalize=True), K)
        e = _trainer(amd, pol, K, seed, _options(), I.im_options(), **RESETS)
        e.teach_days("fixed", T)
        rec = e.rollout_fetch()
        e.close()
        _inputs[name] = rec["obs"].reshape(T * N, -1).copy(), rec["action"].reshape(T * N, -1).copy()
    return _inputs[name]


def _collected(amd, name, opts, im):
    """the shape's policy conditioned on its teacher days (tests/test_imitation_host.py::conditioned), a trainer over it with the
    days recorded and the returns formed: (policy, engine, record, adv, ret, c, ma)"""
    K, seed = W.SHAPES[name]["K"], IM_SEED[name]
    obs, action = _teacher_inputs(amd, name)
    pol = _normed(W.pg_policy(np.random.default_rng(seed), name, normalize=True), K)
    conditioned(pol, obs, action)
    e = _trainer(amd, pol, K, seed, opts, im, **RESETS)
    _assert_state(e.pg_state(), _fresh_state(pol), "theta starts as the device's weights")
    e.teach_days("fixed", T)
    rec = e.rollout_fetch(bootstrap=bool(pol.value_layers))
    assert _same(rec["obs"].reshape(T * N, -1), obs) and _same(rec["action"].reshape(T * N, -1), action)
    done = rec["terminated"] | rec["truncated"]
    assert done[:-1].any() and not done.all(), "a return was meant to be cut inside the record"
    boot = rec["bootstrap_value"] if pol.value_layers else np.zeros(N, F)           # (without a value network every value is +0)
    adv, ret = e.im_advantages(fetch=True)
    radv, rret = I.returns(rec["reward"], rec["terminated"], rec["truncated"], rec["value"], boot, **opts)
    assert _same(adv, radv) and _same(ret, rret)
    ma, c = I.scale(im["ma_start"], radv, **im)
    if im["beta"] > 0:
        w = I.weight(radv, c, **im)
        assert (w == F(im["w_max"])).any() and (w < F(im["w_max"])).any(), "the case was meant to cap some weights and not others"
    return pol, e, rec, radv, rret, c, ma


def _samples(rec, adv, ret):
    """im_ref.grad's sample arrays of all envs: sample s = t * N + env"""
    flat = lambda a: np.ascontiguousarray(a).reshape((-1,) + a.shape[2:])
    return flat(rec["obs"]), flat(rec["action"]), flat(adv), flat(ret), flat(rec["value"])


@pytest.mark.parametrize("name", NAMES)
def test_im_two_minibatch_steps_equal_the_restatement(amd, name):
    """all envs, then the inner range (2, 5) from the moved weights: theta, m, v, the step count and every statistic after each,
    and the moving scale"""
    opts, im = _options(), I.im_options(**W_IM[name])
    pol, e, rec, adv, ret, c, ma = _collected(amd, name, opts, im)
    state = _fresh_state(pol)
    for n0, B in ((0, N), (2, 5)):
        stats = e.im_minibatch(n0, B)
        state, rstats = I.minibatch(pol, state, rec, adv, ret, c, n0, B, opts, im)
        _assert_state(e.pg_state(), state, (n0, B))
        _assert_stats(stats, rstats, (n0, B))
        assert stats["steps"] == state["steps"] and stats["samples"] == T * B
    assert np.isfinite(state["theta"]).all() and not _same(state["theta"], P.flat_params(pol))
    st = e.im_state()
    assert _same(np.float64(st["ma"]), np.float64(ma)) and st["calls"] == 1
    e.close()


@pytest.mark.parametrize("name", NAMES)
def test_im_device_gradient_against_pytorch_autograd(amd, name):
    """One Adam step with beta1 = 0 and no norm clip from fresh moments: m = 0 * 0 + 1 * g, the kernels' gradient itself.  It is
    the restatement's bit for bit, and against float64 autograd of the imitation loss on the record the device produced it meets
    learner_shapes.yardstick over the whole vector and in every term: at most twice float32 autograd's own error.  The inputs'
    conditions are the host test's, asserted on that record: max |z| <= 6, every term alive, no relu on its kink."""
    import torch
    opts, im = _options(beta1=0.0, max_grad_norm=0.0), I.im_options(**W_IM[name])
    pol, e, rec, adv, ret, c, _ = _collected(amd, name, opts, im)
    e.im_minibatch(0, N)
    g = e.pg_state()["m"]
    e.close()
    obs, action, adv, ret, value = _samples(rec, adv, ret)
    theta = P.flat_params(pol)
    rg, _, _ = I.grad(pol, theta, obs, action, adv, ret, value, c, **im)
    assert np.array_equal(g, rg)
    terms = W.pg_terms(pol)
    W.assert_terms_alive(g, terms, name)
    worst = float(np.abs(z64(pol, theta, obs, action)).max())
    print(f"{name} IM device: max |z| {worst:.3f}")
    assert worst <= Z_MAX
    if pol.activation == "relu":
        assert W.relu_margin(obs, pol.layers, pol.value_layers) > 1e-6, "a relu pre-activation sits on its kink: choose another seed"
    if name == "W3":                                                   # (train_log_std = 0: the log-std head's columns are +0)
        A = pol.num_keywords + 1
        (_, wa, wb), (_, ba, bb) = terms[-2], terms[-1]
        for part in (g[wa:wb].reshape(-1, 2 * A)[:, A:], g[ba:bb][A:]):
            assert not part.any() and not np.signbit(part).any(), "the log-std head was not to be trained"
    g64 = _torch_im_grad(pol, theta, obs, action, adv, ret, c, torch.float64, im)
    g32 = _torch_im_grad(pol, theta, obs, action, adv, ret, c, torch.float32, im)
    W.yardstick(f"{name} IM device", g, g64, g32, terms)


def test_im_trains_at_the_last_k_that_fits(amd):
    """hidden (256, 256, 256) for the policy and the value network, two heads, at the largest K whose sample fits 16384 floats of
    LDS: k_im_sample's launch with the whole carve.  Two teacher days of two envs, one MARWIL step over the four samples: the
    restatement's bits"""
    K, seed, envs, days = W.boundary_K("pg"), 61, 2, 2
    assert W.widest_count("pg", K) <= W.LDS_FLOATS < W.widest_count("pg", K + 1)
    pol = W.widest_policy(np.random.default_rng(seed), K, two=True, value=True, log_std_clamp=(-2.0, -0.5))
    pol.layers[-1][1][K + 1:] += F(-1.25)
    opts, im = _options(), I.im_options(beta=0.7, w_max=1.5, ma_rate=1.0)
    e = _trainer(amd, pol, K, seed, opts, im, envs=envs, days=days)
    e.teach_days("fixed", days)
    rec = e.rollout_fetch(bootstrap=True)
    assert rec["obs"].shape == (days, envs, 5 * K + 2)
    adv, ret = e.im_advantages(fetch=True)
    radv, rret = I.returns(rec["reward"], rec["terminated"], rec["truncated"], rec["value"], rec["bootstrap_value"], **opts)
    assert _same(adv, radv) and _same(ret, rret)
    ma, c = I.scale(im["ma_start"], radv, **im)
    stats = e.im_minibatch(0, envs)
    state, rstats = I.minibatch(pol, _fresh_state(pol), rec, radv, rret, c, 0, envs, opts, im)
    _assert_state(e.pg_state(), state)
    _assert_stats(stats, rstats)
    assert stats["samples"] == days * envs and np.isfinite(state["theta"]).all() and not _same(state["theta"], P.flat_params(pol))
    assert _same(np.float64(e.im_state()["ma"]), np.float64(ma))
    e.close()
