"""Policy-gradient trainers for the device-resident MLP policy: PPO (Schulman, Wolski, Dhariwal, Radford, Klimov 2017,
"Proximal Policy Optimization Algorithms") with generalised advantage estimation (Schulman, Moritz, Levine, Jordan, Abbeel
2016), and A2C (Mnih et al. 2016) as its one-epoch, unclipped, single-minibatch special case.  Everything runs on the device:
`run_days("mlp")` records the rollout, `pg_update` computes advantages, the networks' backward pass, the loss and the Adam
step, and writes the new weights where the next day's policy kernel reads them - the record never leaves HBM and an iteration
moves a few hundred bytes of statistics over the bus.  The arithmetic is csrc/adc_pg.h; StepEngine.pg_* are the calls.

The flat parameter order theta[Q]: the policy layers (each W [n_in, n_out] input-major, then b), the value layers in the same
form, then log_std when the policy ends in K+1 means."""
import copy

import numpy as np


def flat_params(policy):
    """theta of an MLPPolicy in the trainer's flat order"""
    parts = [np.concatenate([w.reshape(-1), b]) for w, b in list(policy.layers) + list(policy.value_layers)]
    if policy.log_std is not None:
        parts.append(policy.log_std)
    return np.concatenate(parts).astype(np.float32)


def policy_from_flat(policy, theta):
    """a copy of `policy` (its normalisation and options shared) whose policy layers, value layers and log_std are cut from theta"""
    theta = np.asarray(theta, dtype=np.float32).reshape(-1)
    if theta.size != flat_params(policy).size:
        raise ValueError("policy_from_flat: theta's length is not the policy's parameter count")
    out, o = copy.copy(policy), 0
    nets = []
    for net in (policy.layers, policy.value_layers):
        layers = []
        for w, b in net:
            layers.append((theta[o:o + w.size].reshape(w.shape).copy(), theta[o + w.size:o + w.size + b.size].copy()))
            o += w.size + b.size
        nets.append(layers)
    out.layers, out.value_layers = nets
    if policy.log_std is not None:
        out.log_std = theta[o:o + policy.log_std.size].copy()
    return out


def ppo(**overrides):
    """PPO-clip's usual configuration (Stable-Baselines3's defaults where it has one): 10 epochs over 4 minibatches"""
    cfg = dict(epochs=10, minibatches=4, gamma=0.99, lam=0.95, eps_clip=0.2, vf_coef=0.5, ent_coef=0.0, normalize_advantages=True,
               max_grad_norm=0.5, optimiser="adam", lr=3e-4)
    cfg.update(overrides)
    return cfg


def a2c(**overrides):
    """A2C: one epoch, no clip, one minibatch, un-normalised advantages, lambda 1"""
    cfg = dict(epochs=1, minibatches=1, gamma=0.99, lam=1.0, eps_clip=0.0, vf_coef=0.5, ent_coef=0.0, normalize_advantages=False,
               max_grad_norm=0.5, optimiser="adam", lr=7e-4)
    cfg.update(overrides)
    return cfg


class PGTrainer:
    """engine: a StepEngine that has been reset; policy: the MLPPolicy to start from (collected stochastically whatever its
    own flag says); horizon: the days of one rollout.  config: ppo() / a2c() or keywords of their kind - `epochs`,
    `minibatches` (must divide the engine's envs) and StepEngine.pg_config's options."""

    def __init__(self, engine, policy, horizon, agent_seeds=None, **config):
        cfg = ppo(**config)
        self.epochs, minibatches = int(cfg.pop("epochs")), int(cfg.pop("minibatches"))
        if minibatches < 1 or engine.num_envs % minibatches:
            raise ValueError("minibatches must divide the engine's envs")
        self.engine, self._template, self.horizon = engine, policy, int(horizon)
        self.config = dict(cfg, minibatch_envs=engine.num_envs // minibatches)
        engine.mlp_init(policy, seeds=agent_seeds, deterministic=False)
        engine.rollout_enable(self.horizon, obs=True)
        engine.pg_init(**self.config)
        self.history = []

    def iteration(self, days=None, budget=0.0, reset=False, reset_seeds=None):
        """(reset), `days` (default: the horizon) recorded days of run_days("mlp"), the update; returns its statistics.
        budget > 0 overrides the policy's own budget action."""
        e = self.engine
        if reset:
            e.reset(seeds=reset_seeds)
        e.rollout_reset()
        e.run_days("mlp", self.horizon if days is None else int(days), budget)
        stats = e.pg_update(self.epochs)
        self.history.append(stats)
        return stats

    def policy(self):
        """an MLPPolicy holding the trained policy layers, value layers and log_std"""
        return policy_from_flat(self._template, self.engine.pg_state()["theta"])

    def state(self, state=None):
        return self.engine.pg_state(state)


__all__ = ["PGTrainer", "ppo", "a2c", "flat_params", "policy_from_flat"]
