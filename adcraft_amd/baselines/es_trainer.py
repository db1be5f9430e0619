"""An evolution-strategy trainer for the device-resident MLP policy (OpenAI-ES: Salimans, Ho, Chen, Sidor, Sutskever 2017,
"Evolution Strategies as a Scalable Alternative to Reinforcement Learning"): antithetic Gaussian parameter noise, centred-rank
fitness shaping, Adam on the estimated gradient.  Everything runs on the device - the members' weights are perturbed from
counter-addressed noise, a generation is one `run_days("mlp")`, the update regenerates the noise - so a generation moves a few
kilobytes over the bus (the per-env returns and the statistics), whatever the population's size.  The arithmetic is
csrc/adc_es.h; StepEngine.es_* are the calls.

The defaults (sigma 0.02, Adam lr 0.01) are the paper's; nobody has tuned them on this env."""
import copy

import numpy as np


def _terms(policy):
    """the (W, b) pairs of the flat order: the layers, a recurrent policy's (Wi, bi), (Wh, bh) in front of its output layer"""
    gru = getattr(policy, "gru", None)
    if gru is None:
        return list(policy.layers)
    return list(policy.layers[:-1]) + [(gru[0], gru[1]), (gru[2], gru[3]), policy.layers[-1]]


def flat_params(policy):
    """the policy network's parameters in the engine's flat order: layers in order, each W [n_in, n_out] input-major
    (j * n_out + h) followed by its b; a recurrent policy's cell - Wi, bi, Wh, bh - stands in front of its output layer"""
    return np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b in _terms(policy)]).astype(np.float32)


def policy_from_flat(policy, flat):
    """a copy of `policy` (its value network, log_std, normalisation and options shared) whose policy layers are cut from `flat`"""
    flat = np.asarray(flat, dtype=np.float32).reshape(-1)
    terms = _terms(policy)
    if flat.size != sum(w.size + b.size for w, b in terms):
        raise ValueError("policy_from_flat: the flat vector's length is not the policy network's parameter count")
    out, o, cut = copy.copy(policy), 0, []
    for w, b in terms:
        cut.append((flat[o:o + w.size].reshape(w.shape).copy(), flat[o + w.size:o + w.size + b.size].copy()))
        o += w.size + b.size
    if getattr(policy, "gru", None) is None:
        out.layers = cut
    else:
        out.layers = cut[:-3] + [cut[-1]]
        out.gru = cut[-3] + cut[-2]
    return out


def default_policy(num_keywords, hidden=(32, 32), days=60, seed=0, log_std=-2.0, deterministic=True, frames=1, gru=0):
    """the untrained `[32, 32]` tanh policy of examples/evaluate_mlp_policy.py, built in numpy: every Linear layer drawn uniformly
    in +-1 / sqrt(n_in) (weights and biases), the last layer's weights scaled by 0.1 and its biases set to 0.5 - an agent that
    bids about 50 cents everywhere - on observations scaled to O(1) (counts and dollars * 0.1, cumulative profit * 1e-3,
    days / `days`).  frames: the observations its input row holds (MLPPolicy(frames=...)); every frame is scaled alike.
    gru = G > 0: a recurrent policy, a GRU cell of width G in front of the output layer, the cell
    drawn uniformly in +-1 / sqrt(G) as torch.nn.GRUCell is"""
    from .mlp_policy import MLPPolicy
    rng = np.random.default_rng(seed)
    K = int(num_keywords)
    D0, A = 5 * K + 2, K + 1
    D = int(frames) * D0
    layers, n_in, cell, G = [], D, None, int(gru)
    for i, n_out in enumerate(list(hidden) + [A]):
        if G and i == len(hidden):
            bound = 1.0 / np.sqrt(G)
            cell = tuple(rng.uniform(-bound, bound, shape).astype(np.float32) for shape in ((n_in, 3 * G), (3 * G,), (G, 3 * G), (3 * G,)))
            n_in = G
        bound = 1.0 / np.sqrt(n_in)
        layers.append([rng.uniform(-bound, bound, (n_in, n_out)).astype(np.float32), rng.uniform(-bound, bound, n_out).astype(np.float32)])
        n_in = n_out
    layers[-1][0] *= np.float32(0.1)
    layers[-1][1][:] = 0.5
    scale = np.full(D0, 0.1, np.float32)
    scale[2 * K], scale[2 * K + 1] = 1.0e-3, 1.0 / days
    return MLPPolicy([tuple(l) for l in layers], shift=np.zeros(D, np.float32), scale=np.tile(scale, int(frames)), log_std=np.full(A, log_std, np.float32),
                     deterministic=deterministic, frames=int(frames), gru=cell)


class ESTrainer:
    """engine: a StepEngine that has been reset; policy: the MLPPolicy to start from (the centre); members: an even number
    dividing the engine's envs (member m evaluates on envs m * N / members ...), or pass member_of_env.  Further options are
    StepEngine.es_config's (beta1, beta2, eps, l2, shaping, optimiser, seed)."""

    def __init__(self, engine, policy, members, sigma=0.02, lr=0.01, member_of_env=None, agent_seeds=None, **options):
        self.engine, self._template, self.members = engine, policy, int(members)
        engine.mlp_init(policy, seeds=agent_seeds)
        engine.mlp_population(self.members, member_of_env)
        engine.es_init(sigma=sigma, lr=lr, **options)
        self.history = []

    def generation(self, days, budget=0.0, reset=True, reset_seeds=None):
        """perturb, (reset), `days` days of run_days("mlp"), update; returns the update's statistics.  budget > 0 overrides
        the policy's own budget action."""
        e = self.engine
        e.es_perturb()
        if reset:
            e.reset(seeds=reset_seeds)
        e.run_days("mlp", int(days), budget)
        stats = e.es_update()
        self.history.append(stats)
        return stats

    def policy(self):
        """an MLPPolicy holding the current centre"""
        return policy_from_flat(self._template, self.engine.mlp_params())

    def state(self, state=None):
        """get (no argument) or set the strategy's state; the observation history (`obs_history`) and a recurrent policy's
        state (`hidden`) ride along, so that a resumed run continues bit for bit"""
        from .mlp_policy import history_carry
        e = self.engine
        if state is None:
            st = history_carry(e, e.es_state, None)
            hidden = e.mlp_hidden_state()
            if hidden is not None:
                st["hidden"] = hidden
            return st
        state = dict(state)
        hidden = state.pop("hidden", None)
        out = history_carry(e, e.es_state, state)
        if hidden is not None or e.mlp_gru_width():
            e.mlp_set_hidden_state(hidden)
        return out


__all__ = ["ESTrainer", "default_policy", "flat_params", "policy_from_flat"]
