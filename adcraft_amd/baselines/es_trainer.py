"""An evolution-strategy trainer for the device-resident MLP policy (OpenAI-ES: Salimans, Ho, Chen, Sidor, Sutskever 2017,
"Evolution Strategies as a Scalable Alternative to Reinforcement Learning"): antithetic Gaussian parameter noise, centred-rank
fitness shaping, Adam on the estimated gradient.  Everything runs on the device - the members' weights are perturbed from
counter-addressed noise, a generation is one `run_days("mlp")`, the update regenerates the noise - so a generation moves a few
kilobytes over the bus (the per-env returns and the statistics), whatever the population's size.  The arithmetic is
csrc/adc_es.h; StepEngine.es_* are the calls.

The defaults (sigma 0.02, Adam lr 0.01) are the paper's; nobody has tuned them on this env."""
import copy

import numpy as np


def flat_params(policy):
    """the policy network's parameters in the engine's flat order: layers in order, each W [n_in, n_out] input-major
    (j * n_out + h) followed by its b"""
    return np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b in policy.layers]).astype(np.float32)


def policy_from_flat(policy, flat):
    """a copy of `policy` (its value network, log_std, normalisation and options shared) whose policy layers are cut from `flat`"""
    flat = np.asarray(flat, dtype=np.float32).reshape(-1)
    if flat.size != sum(w.size + b.size for w, b in policy.layers):
        raise ValueError("policy_from_flat: the flat vector's length is not the policy network's parameter count")
    out, o, layers = copy.copy(policy), 0, []
    for w, b in policy.layers:
        layers.append((flat[o:o + w.size].reshape(w.shape).copy(), flat[o + w.size:o + w.size + b.size].copy()))
        o += w.size + b.size
    out.layers = layers
    return out


def default_policy(num_keywords, hidden=(32, 32), days=60, seed=0, log_std=-2.0, deterministic=True, frames=1):
    """the untrained `[32, 32]` tanh policy of examples/evaluate_mlp_policy.py, built in numpy: every Linear layer drawn uniformly
    in +-1 / sqrt(n_in) (weights and biases), the last layer's weights scaled by 0.1 and its biases set to 0.5 - an agent that
    bids about 50 cents everywhere - on observations scaled to O(1) (counts and dollars * 0.1, cumulative profit * 1e-3,
    days / `days`).  frames: the observations its input row holds (MLPPolicy(frames=...)); every frame is scaled alike"""
    from .mlp_policy import MLPPolicy
    rng = np.random.default_rng(seed)
    K = int(num_keywords)
    D0, A = 5 * K + 2, K + 1
    D = int(frames) * D0
    layers, n_in = [], D
    for n_out in list(hidden) + [A]:
        bound = 1.0 / np.sqrt(n_in)
        layers.append([rng.uniform(-bound, bound, (n_in, n_out)).astype(np.float32), rng.uniform(-bound, bound, n_out).astype(np.float32)])
        n_in = n_out
    layers[-1][0] *= np.float32(0.1)
    layers[-1][1][:] = 0.5
    scale = np.full(D0, 0.1, np.float32)
    scale[2 * K], scale[2 * K + 1] = 1.0e-3, 1.0 / days
    return MLPPolicy([tuple(l) for l in layers], shift=np.zeros(D, np.float32), scale=np.tile(scale, int(frames)), log_std=np.full(A, log_std, np.float32),
                     deterministic=deterministic, frames=int(frames))


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
        from .mlp_policy import history_carry
        return history_carry(self.engine, self.engine.es_state, state)


__all__ = ["ESTrainer", "default_policy", "flat_params", "policy_from_flat"]
