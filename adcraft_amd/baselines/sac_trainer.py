"""Soft actor-critic (Haarnoja et al. 2018, "Soft Actor-Critic Algorithms and Applications") for the device-resident MLP
policy: a tanh-squashed Gaussian actor, twin critics with Polyak targets and a learned temperature, over the replay ring that
lives on the device.  `run_days("mlp")` records the rollout under the squashed act, `sac_store` appends it to the ring,
`sac_update` trains the critics, the actor and the temperature and writes the new actor where the next day's policy kernel
reads it: collect -> store -> update runs without a transition leaving HBM.  The arithmetic is csrc/adc_sac.h;
StepEngine.sac_* and StepEngine.mlp_set_squash are the calls.

The actor is the MLPPolicy's policy network with two heads (means, then log-stds) and the log-std clamp; the env is given
lo + 0.5 (hi - lo) (tanh(u) + 1) for the sampled u, so the bounds (action_lo, action_hi) are the range of budgets and bids the
agent can reach.  Exploration is the policy's own noise: there is no exploration sigma to set."""
import copy

import numpy as np

from .td3_trainer import policy_from_actor, random_critics


def sac(num_keywords, **overrides):
    """RLlib's SAC defaults: gamma 0.99, tau 5e-3, the targets every update, the three learning rates 3e-4, alpha starting at 1
    with the target entropy -(K + 1), batches of 256, critics of two hidden layers of 256"""
    cfg = dict(critic_hidden=(256, 256), learning_starts=1500, updates_per_iteration=64, gamma=0.99, tau=5e-3, target_update_interval=1,
               init_alpha=1.0, target_entropy=-float(num_keywords + 1), alpha_lr=3e-4, batch_size=256, capacity=1000000, actor_lr=3e-4,
               critic_lr=3e-4, optimiser="adam")
    cfg.update(overrides)
    return cfg


class SquashedPolicy:
    """what SACTrainer.policy() exports: the trained MLPPolicy and the squash bounds that belong to its actions"""

    def __init__(self, policy, action_lo, action_hi):
        self.policy, self.action_lo, self.action_hi = policy, np.array(action_lo, np.float32), np.array(action_hi, np.float32)

    def install(self, engine, seeds=None, deterministic=None):
        """the policy and its bounds onto an engine: mlp_init, then mlp_set_squash"""
        engine.mlp_init(self.policy, seeds=seeds, deterministic=deterministic)
        engine.mlp_set_squash(self.action_lo, self.action_hi)


class SACTrainer:
    """engine: a StepEngine that has been reset; policy: the MLPPolicy to start from (2 (K + 1) outputs, log_std_clamp set; a
    value network is ignored); action_lo / action_hi [K + 1] (or scalars): the squash bounds in the flat action order (budget,
    bids); critic_hidden: the critics' hidden widths (each <= 256); horizon: the days of one collection; learning_starts:
    transitions the ring must hold before the first update; updates_per_iteration: updates after every collection.  config:
    sac()'s other keys and StepEngine.sac_config's options, plus critic_seed (random_critics' seed) and critics (two lists of
    layers, instead)."""

    def __init__(self, engine, policy, action_lo, action_hi, critic_hidden=(256, 256), horizon=10, learning_starts=1500, updates_per_iteration=64,
                 agent_seeds=None, **config):
        A = policy.num_keywords + 1
        if policy.output_size != 2 * A or policy.log_std_clamp is None:
            raise ValueError("SAC needs a policy that ends in 2 (K + 1) outputs (means, log-stds) with log_std_clamp set")
        cfg = dict(config)
        critics, critic_seed = cfg.pop("critics", None), cfg.pop("critic_seed", 0)
        self.engine, self.horizon = engine, int(horizon)
        self.learning_starts, self.updates_per_iteration = int(learning_starts), int(updates_per_iteration)
        self.action_lo, self.action_hi = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32), (A,))) for v in (action_lo, action_hi))
        self._template = copy.copy(policy)
        self.config = dict(cfg, critic_widths=tuple(critic_hidden) + (1,))
        engine.mlp_init(self._template, seeds=agent_seeds, deterministic=False)
        engine.mlp_set_squash(self.action_lo, self.action_hi)
        engine.rollout_enable(self.horizon, obs=True)
        engine.sac_init(**self.config)
        engine.sac_set_critics(critics if critics is not None else random_critics(policy.num_keywords, critic_hidden, critic_seed))
        self.history = []

    def iteration(self, days=None, budget=0.0, reset=False, reset_seeds=None):
        """(reset), `days` (default: the horizon) recorded days of run_days("mlp"), the store, and - once the ring holds
        learning_starts transitions - updates_per_iteration updates; returns their statistics, or only the ring's size before
        that.  budget > 0 overrides the policy's own (squashed) budget action."""
        e = self.engine
        if reset:
            e.reset(seeds=reset_seeds)
        e.rollout_reset()
        e.run_days("mlp", self.horizon if days is None else int(days), budget)
        e.sac_store()
        size = e.sac_buffer(fetch=False)["size"]
        stats = e.sac_update(self.updates_per_iteration) if size >= self.learning_starts else dict(buffer_size=size, updates=None)
        self.history.append(stats)
        return stats

    def policy(self):
        """the trained actor with the squash bounds its actions are meant under"""
        return SquashedPolicy(policy_from_actor(self._template, self.engine.sac_state()["theta"]), self.action_lo, self.action_hi)

    def state(self, state=None):
        return self.engine.sac_state(state)
