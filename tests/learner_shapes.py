"""The network shapes at which the learner kernels' shape-dependent structures take another path, shared by
tests/test_learner_shapes_host.py and tests/test_gpu_learner_shapes.py: the shapes W1-W3 and their policies and critics, the
library's LDS float counts restated, and the float64-autograd yardstick of tests/test_pg_host.py as a function.

A per-sample workgroup has 256 lanes, eight per neuron: a layer loop covers 32 neurons a pass.  Weights sit in blocks of 32
inputs read in chains of 8; the weight gradient is cut into 16 x 16 tiles with the bias as row n_in; head loops stride by 256.

  W1  K = 40  (D 202, A 41)   tanh, hidden (256, 255, 33), a free log_std under a clamp that moves some components; a value network
                              of another depth, hidden (33,); critics (255, 33, 7, 1).  8 passes of a layer loop; the ragged widths
                              255 and 33 (chains, blocks, tiles); n_in = 256 and 32 (the bias row alone in its tile row); 41 action
                              inputs (2 passes of td3_input_back)
  W2  K = 130 (D 652, A 131)  relu, two heads (262 outputs, wider than the widest hidden layer allowed), hidden (33, 250, 64): four
                              layers; a value network of hidden (256, 256, 256); critics (256, 256, 256, 1).  The deepest and
                              widest networks; maxw = 2 A; 5 passes over A
  W3  K = 256 (D 1282, A 257) tanh, two heads (514 outputs), hidden (31,), no value network; critics (32, 1).  A > 256: every loop
                              a = tid; a < A; a += 256 wraps; a layer one lane short of a full pass
"""
import numpy as np

from tests import mlp_ref as R
from tests import sac_ref as S
from tests import td3_ref as T3

F = np.float32
LDS_FLOATS = 16384                                                     # 64 KiB
WIDEST = dict(hidden=(256, 256, 256), critics=(256, 256, 256, 1))

SHAPES = dict(
    W1=dict(K=40, act="tanh", hidden=(256, 255, 33), two=False, clamp=(-1.5, -0.5), value_hidden=(33,), critics=(255, 33, 7, 1)),
    W2=dict(K=130, act="relu", hidden=(33, 250, 64), two=True, clamp=None, value_hidden=(256, 256, 256), critics=(256, 256, 256, 1)),
    W3=dict(K=256, act="tanh", hidden=(31,), two=True, clamp=None, value_hidden=None, critics=(32, 1)),
)


def pg_policy(rng, name, scale=0.6, **kw):
    """the PPO / A2C policy of a shape: the value network drawn on its own widths; W1's free log_std on both sides of both bounds"""
    s = SHAPES[name]
    K = s["K"]
    pol = R.random_policy(rng, K, s["hidden"], s["act"], two_heads=s["two"], value=False, scale=scale, log_std_clamp=s["clamp"], **kw)
    if s["value_hidden"] is not None:
        pol.value_layers = R.random_policy(rng, K, s["value_hidden"], s["act"], value=True, scale=scale).value_layers
    if s["clamp"] is not None and not s["two"]:
        pol.log_std = np.linspace(s["clamp"][0] - 0.5, s["clamp"][1] + 0.5, K + 1).astype(F)
    if s["two"]:
        # the log-std head around -1.42, where a component's expected log-probability term -z^2/2 - ls - log(2 pi)/2 is zero: log p
        # is then O(sqrt(A)), not O(A).  Around ls = 0, log p is near -1.42 A (-190 at W2, -365 at W3) and its own float32 rounding,
        # 1e-5 of the ratio and common to the law and to float32 autograd, is all that the autograd yardstick would compare
        pol.layers[-1][1][K + 1:] += F(-1.42)
    return pol


def td3_policy(rng, name, scale=0.6, **kw):
    """the TD3 actor of a shape: one head (a two-headed policy has no TD3 shape), the shape's hidden widths"""
    s = SHAPES[name]
    return R.random_policy(rng, s["K"], s["hidden"], s["act"], scale=scale, **kw)


def sac_policy(rng, name, scale=0.6, clamp=(-1.0, -0.5), **kw):
    """the SAC actor of a shape: two heads under the clamp, the log-std head's biases from below its lower bound to above its upper"""
    s = SHAPES[name]
    K = s["K"]
    pol = S.sac_policy(rng, K, s["hidden"], s["act"], clamp=clamp, scale=scale, **kw)
    pol.layers[-1][1][K + 1:] = np.linspace(clamp[0] - 0.6, clamp[1] + 0.6, K + 1).astype(F)
    return pol


def critics(rng, name, scale=0.6):
    return T3.random_critics_for_tests(rng, SHAPES[name]["K"], SHAPES[name]["critics"], scale=scale)


def widest_policy(rng, K, two, value, frames=1, scale=0.3, **kw):
    """hidden (256, 256, 256) for the policy (and the value network): the most LDS a sample of K keywords can ask for"""
    from tests import stack_ref
    if frames > 1:
        return stack_ref.random_policy(rng, K, frames, WIDEST["hidden"], "tanh", two_heads=two, value=value, scale=scale, **kw)
    return R.random_policy(rng, K, WIDEST["hidden"], "tanh", two_heads=two, value=value, scale=scale, **kw)


# ---- the library's LDS counts, restated (kernel_pg.inc pg_lds_floats, kernel_td3.inc td3_lds_floats, kernel_sac.inc sac_lds_floats) ----
def pg_lds_floats(K, pol_widths, val_widths, kl=False, frames=1):
    """x | every layer's outputs of both networks | two delta rows of the widest layer | z, sd, ls (kl: and mean_old, ls_old)"""
    D, A = frames * (5 * K + 2), K + 1
    maxw = max([1] + list(pol_widths) + list(val_widths))
    return D + 2 * maxw + (5 if kl else 3) * A + sum(pol_widths) + sum(val_widths)


def td3_lds_floats(K, pol_widths, q_widths, frames=1):
    """row | the actor's outputs | one critic's outputs | two delta rows and a dump row | four words"""
    D, A = frames * (5 * K + 2), K + 1
    maxw = max([A] + list(pol_widths) + list(q_widths))
    return D + A + sum(pol_widths) + sum(q_widths) + 3 * maxw + 4


def sac_lds_floats(K, pol_widths, q_widths, frames=1):
    """row | the actor's outputs | both critics' outputs | two delta rows and a dump row | six head vectors | eight words"""
    D, A = frames * (5 * K + 2), K + 1
    maxw = max([A] + list(pol_widths) + list(q_widths))
    return D + A + sum(pol_widths) + 2 * sum(q_widths) + 3 * maxw + 6 * A + 8


def widest_count(family, K, frames=1):
    """the float count of a sample of K keywords under the widest networks of the family; frames: the stacked row's D = frames (5 K + 2)"""
    h, q, A = list(WIDEST["hidden"]), list(WIDEST["critics"]), K + 1
    if family in ("pg", "pg_kl"):
        return pg_lds_floats(K, h + [2 * A], h + [1], kl=family == "pg_kl", frames=frames)
    if family == "td3":
        return td3_lds_floats(K, h + [A], q, frames)
    return sac_lds_floats(K, h + [2 * A], q, frames)


def boundary_K(family, frames=1):
    """the largest K whose sample fits 64 KiB of LDS (the count grows with K)"""
    K = 1
    while widest_count(family, K + 1, frames) <= LDS_FLOATS:
        K += 1
    assert widest_count(family, K, frames) <= LDS_FLOATS < widest_count(family, K + 1, frames)
    return K


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
def pg_terms(pol):
    """(name, begin, end) of every term of pg_ref's flat order: each layer's weights, each layer's biases, log_std"""
    terms, pos = [], 0
    for name, net in (("policy", pol.layers), ("value", pol.value_layers)):
        for l, (w, b) in enumerate(net):
            terms += [(f"{name} W{l}", pos, pos + w.size), (f"{name} b{l}", pos + w.size, pos + w.size + b.size)]
            pos += w.size + b.size
    if pol.log_std is not None:
        terms.append(("log_std", pos, pos + pol.log_std.size))
    return terms


def net_terms(name, n_in, widths, pos=0):
    terms = []
    for l, n_out in enumerate(widths):
        terms += [(f"{name} W{l}", pos, pos + n_in * n_out), (f"{name} b{l}", pos + n_in * n_out, pos + (n_in + 1) * n_out)]
        pos += (n_in + 1) * n_out
        n_in = n_out
    return terms


def offpolicy_terms(sh):
    """(the critics' terms over psi's gradient [2 Qc], the actor's over theta's [P])"""
    c = net_terms("critic1", sh.D + sh.A, sh.q_widths) + net_terms("critic2", sh.D + sh.A, sh.q_widths, sh.Qc)
    return c, net_terms("actor", sh.D, sh.pol_widths)


def assert_terms_alive(g, terms, what=""):
    """every term of the gradient is finite and has a nonzero entry: a case cannot pass on zeros"""
    g = np.asarray(g)
    assert np.isfinite(g).all(), what
    assert terms[-1][2] == g.size, (what, terms[-1][2], g.size)
    dead = [name for name, a, b in terms if not np.abs(g[a:b]).max() > 0]
    assert not dead, (what, dead)


def yardstick(what, g, g64, g32, terms, log=print):
    """tests/test_pg_host.py's yardstick: the error of g against float64 autograd (largest absolute difference over the largest
    float64 entry) is at most twice float32 autograd's own on the same arrays, over the whole vector and in every term on its
    own, the per-term yardstick not taken below 2^-23.  Prints every figure, then asserts; returns the whole vector's
    (error, float32 autograd's error)"""
    g, g32 = np.asarray(g, np.float64), np.asarray(g32, np.float64)
    assert g.shape == g64.shape == g32.shape, (what, g.shape, g64.shape)
    scale = np.abs(g64).max()
    err, err32 = np.abs(g - g64).max() / scale, np.abs(g32 - g64).max() / scale
    log(f"{what} whole ({g.size} parameters): error {err:.3e}  float32 autograd {err32:.3e}  ratio {err / err32:.3f}")
    failed = []
    for name, a, b in terms:
        scale = np.abs(g64[a:b]).max()
        assert scale > 0, (what, name)
        e, e32 = np.abs(g[a:b] - g64[a:b]).max() / scale, np.abs(g32[a:b] - g64[a:b]).max() / scale
        log(f"{what} {name:12s}: error {e:.3e}  float32 autograd {e32:.3e}  ratio {e / e32 if e32 else float('nan'):.3f}")
        if not e <= 2 * max(e32, 2.0 ** -23):
            failed.append((name, e, e32))
    assert err <= 2 * err32, (what, err, err32)
    assert not failed, (what, failed)
    return err, err32


def relu_margin(x, *nets):
    """the smallest |pre-activation| of any hidden relu of the networks on the rows x, in float64"""
    margin = np.inf
    for layers in nets:
        h = np.asarray(x, np.float64)
        for w, b in layers[:-1]:
            pre = h @ np.asarray(w, np.float64) + np.asarray(b, np.float64)
            margin = min(margin, float(np.abs(pre).min()))
            h = np.maximum(pre, 0.0)
    return margin
