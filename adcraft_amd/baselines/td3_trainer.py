"""TD3 (Fujimoto, van Hoof, Meger 2018, "Addressing Function Approximation Error in Actor-Critic Methods") for the
device-resident MLP policy: the deterministic policy gradient (Lillicrap et al. 2016) with twin critics, clipped target
smoothing noise and delayed actor / target updates, over a replay ring that lives on the device.  `run_days("mlp")` records the
rollout, `td3_store` appends it to the ring, `td3_update` samples minibatches, trains the critics and - every policy_delay-th
update - the actor, and writes the new actor where the next day's policy kernel reads it: collect -> store -> update runs
without a transition leaving HBM.  The arithmetic is csrc/adc_td3.h; StepEngine.td3_* are the calls.

The actor is the MLPPolicy's policy network with the free log_std head; its mean is the deterministic action and
mean + exp(log_std) * z, log_std = log(exploration sigma), the exploration.  The reference's pure-random warm-up
(`random_timesteps`) is covered by collecting under the initial policy with a larger sigma for the first iterations:
`TD3Trainer.set_exploration(sigma)`, then back."""
import copy

import numpy as np


def td3(**overrides):
    """Fujimoto et al.'s configuration: gamma 0.99, tau 0.005, actor and targets every 2nd update, target noise 0.2 clipped at
    0.5, batches of 256, both learning rates 1e-3, exploration sigma 0.1, critics of two hidden layers of 256"""
    cfg = dict(critic_hidden=(256, 256), exploration_sigma=0.1, learning_starts=10000, updates_per_iteration=64, gamma=0.99, tau=0.005,
               policy_delay=2, target_noise=0.2, target_noise_clip=0.5, batch_size=256, capacity=1000000, actor_lr=1e-3, critic_lr=1e-3,
               optimiser="adam")
    cfg.update(overrides)
    return cfg


def random_critics(K, hidden, seed=0):
    """two critics on the 6K + 3 inputs [x | action] with torch's default Linear initialisation: weights and biases uniform in
    +- 1 / sqrt(n_in)"""
    rng, out = np.random.default_rng(seed), []
    for _ in range(2):
        layers, n_in = [], 6 * K + 3
        for n_out in list(hidden) + [1]:
            bound = 1.0 / np.sqrt(n_in)
            layers.append((rng.uniform(-bound, bound, (n_in, n_out)).astype(np.float32), rng.uniform(-bound, bound, n_out).astype(np.float32)))
            n_in = n_out
        out.append(layers)
    return out


def actor_params(policy):
    """theta of an MLPPolicy: its policy layers, each W [n_in, n_out] input-major, then b"""
    return np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b in policy.layers]).astype(np.float32)


def policy_from_actor(policy, theta):
    """a copy of `policy` whose policy layers are cut from theta"""
    theta = np.asarray(theta, dtype=np.float32).reshape(-1)
    if theta.size != actor_params(policy).size:
        raise ValueError("policy_from_actor: theta's length is not the policy network's parameter count")
    out, o, layers = copy.copy(policy), 0, []
    for w, b in policy.layers:
        layers.append((theta[o:o + w.size].reshape(w.shape).copy(), theta[o + w.size:o + w.size + b.size].copy()))
        o += w.size + b.size
    out.layers = layers
    return out


class TD3Trainer:
    """engine: a StepEngine that has been reset; policy: the MLPPolicy to start from (K + 1 means, free log_std; a value network
    is ignored); critic_hidden: the critics' hidden widths (each <= 256); horizon: the days of one collection;
    exploration_sigma: the standard deviation of the collection noise; learning_starts: transitions the ring must hold before
    the first update; updates_per_iteration: critic updates after every collection.  config: td3()'s other keys and
    StepEngine.td3_config's options, plus critic_seed (random_critics' seed), critics (two lists of layers, instead) and
    action_norm ((shift, scale) [K + 1] for the critics' action inputs)."""

    def __init__(self, engine, policy, critic_hidden=(256, 256), horizon=10, exploration_sigma=0.1, learning_starts=10000, updates_per_iteration=64,
                 agent_seeds=None, **config):
        if policy.log_std is None:
            raise ValueError("TD3 needs a policy that ends in K + 1 means with the free log_std vector")
        cfg = dict(config)
        critics, norm = cfg.pop("critics", None), cfg.pop("action_norm", None)
        critic_seed = cfg.pop("critic_seed", 0)
        self.engine, self.horizon = engine, int(horizon)
        self.learning_starts, self.updates_per_iteration = int(learning_starts), int(updates_per_iteration)
        self._template = copy.copy(policy)
        self._template.log_std = np.full(policy.num_keywords + 1, np.log(exploration_sigma), np.float32)
        self.config = dict(cfg, critic_widths=tuple(critic_hidden) + (1,))
        engine.mlp_init(self._template, seeds=agent_seeds, deterministic=False)
        engine.rollout_enable(self.horizon, obs=True)
        engine.td3_init(**self.config)
        engine.td3_set_critics(critics if critics is not None else random_critics(policy.num_keywords, critic_hidden, critic_seed), action_norm=norm)
        self.history = []

    def set_exploration(self, sigma):
        """the collection noise's standard deviation from the next day on (a larger one for a warm-up's first iterations)"""
        self._template.log_std = np.full(self._template.num_keywords + 1, np.log(sigma), np.float32)
        self.engine.mlp_set_log_std(self._template.log_std)

    def iteration(self, days=None, budget=0.0, reset=False, reset_seeds=None):
        """(reset), `days` (default: the horizon) recorded days of run_days("mlp"), the store, and - once the ring holds
        learning_starts transitions - updates_per_iteration updates; returns their statistics, or only the ring's size before
        that.  budget > 0 overrides the policy's own budget action."""
        e = self.engine
        if reset:
            e.reset(seeds=reset_seeds)
        e.rollout_reset()
        e.run_days("mlp", self.horizon if days is None else int(days), budget)
        e.td3_store()
        size = e.td3_buffer(fetch=False)["size"]
        stats = e.td3_update(self.updates_per_iteration) if size >= self.learning_starts else dict(buffer_size=size, updates=None)
        self.history.append(stats)
        return stats

    def policy(self):
        """an MLPPolicy holding the trained actor (its log_std the exploration's)"""
        return policy_from_actor(self._template, self.engine.td3_state()["theta"])

    def state(self, state=None):
        return self.engine.td3_state(state)


__all__ = ["TD3Trainer", "td3", "random_critics", "actor_params", "policy_from_actor"]
