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

from .mlp_policy import history_carry
from .td3_trainer import (NORM_OPTIONS, NStepReturns, PrioritizedReplay, _norm_options, _norm_state, _with_vectors, nstep_check, policy_from_actor, random_critics,
                          shared_nstep)


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


def _sac_norm_options(policies, normalize_observations, normalize_rewards, norm, config):
    """the normalisers' options: the dict `norm`, or NORM_OPTIONS keys given among a trainer's keyword options (taken out of config)"""
    loose = {k: config.pop(k) for k in NORM_OPTIONS if k in config}
    if loose and norm is not None:
        raise ValueError("the normalisers' options are given either as norm=dict(...) or as keywords, not both")
    return _norm_options(policies, normalize_observations, normalize_rewards, loose or norm)


class _NormalizedSAC:
    """the trainers' side of normalize_observations / normalize_rewards: running normalisers on the device (StepEngine.sac_norm_*;
    csrc/adc_sac_norm.h).  The record and the ring then hold raw observations and raw rewards and every batch is normalised as it is
    sampled, with the statistics updated from every collection BEFORE its updates.  Only the reward is scaled, not the entropy term:
    target_entropy and alpha then trade against a return of about unit standard deviation.  What the normalisers gain in learning
    has not been measured."""

    def _norm_on(self):
        return self.normalize_observations or self.normalize_rewards

    def _norm_carry(self, get_or_set, member, state, envs=None):
        """get_or_set(state): the trainer's own state call; `norm` (the normaliser's moments, vectors, multiplier and the envs' return
        carries) rides along, so that a resumed run continues bit for bit"""
        if state is None:
            st = get_or_set(None)
            if self._norm_on():
                st["norm"] = _norm_state(self.engine, member, None, envs, family="sac")
            return st
        state = dict(state)
        norm = state.pop("norm", None)
        get_or_set(state)
        if norm is not None and self._norm_on():
            _norm_state(self.engine, member, norm, envs, family="sac")


class SACTrainer(PrioritizedReplay, NStepReturns, _NormalizedSAC):
    """engine: a StepEngine that has been reset; policy: the MLPPolicy to start from (2 (K + 1) outputs, log_std_clamp set; a
    value network is ignored); action_lo / action_hi [K + 1] (or scalars): the squash bounds in the flat action order (budget,
    bids); critic_hidden: the critics' hidden widths (each <= 256); horizon: the days of one collection; learning_starts:
    transitions the ring must hold before the first update; updates_per_iteration: updates after every collection.  config:
    sac()'s other keys and StepEngine.sac_config's options, plus critic_seed (random_critics' seed) and critics (two lists of
    layers, instead).  prioritized_replay: None, or PrioritizedReplay's dict (td3_trainer.py).  n_step: the window of n-step
    returns, 1 (off) to 16 (NStepReturns, td3_trainer.py); state() carries `replay_nstep`.

    normalize_observations / normalize_rewards: running normalisers on the device (_NormalizedSAC above); their options -
    obs_min_std, obs_count_cap, rew_min_std, rew_count_cap, rew_clip - as keywords or as norm=dict(...).  state() / load_state()
    carry the normaliser."""

    def __init__(self, engine, policy, action_lo, action_hi, critic_hidden=(256, 256), horizon=10, learning_starts=1500, updates_per_iteration=64,
                 agent_seeds=None, prioritized_replay=None, normalize_observations=False, normalize_rewards=False, norm=None, n_step=1, **config):
        cfg = dict(config)
        n_step = nstep_check(n_step)
        norm = _sac_norm_options([policy], normalize_observations, normalize_rewards, norm, cfg)
        A = policy.num_keywords + 1
        if policy.output_size != 2 * A or policy.log_std_clamp is None:
            raise ValueError("SAC needs a policy that ends in 2 (K + 1) outputs (means, log-stds) with log_std_clamp set")
        self.normalize_observations, self.normalize_rewards = bool(normalize_observations), bool(normalize_rewards)
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
        engine.sac_set_critics(critics if critics is not None else random_critics(policy.num_keywords, critic_hidden, critic_seed, policy.frames))
        if self._norm_on():
            engine.sac_norm_init(observations=self.normalize_observations, rewards=self.normalize_rewards, **norm)
        self._prio_init(engine, prioritized_replay)
        self._nstep_init(engine, n_step)
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
        if self._norm_on():
            e.sac_norm_update()             # (the batches below are scaled by statistics that include the newest days)
        size = e.sac_buffer(fetch=False)["size"]
        if size >= self.learning_starts:
            self._prio_anneal()
        stats = e.sac_update(self.updates_per_iteration) if size >= self.learning_starts else dict(buffer_size=size, updates=None)
        self.history.append(stats)
        return stats

    def policy(self):
        """the trained actor with the squash bounds its actions are meant under"""
        pol = policy_from_actor(self._template, self.engine.sac_state()["theta"])
        if self.normalize_observations:
            pol = _with_vectors(pol, self.engine.sac_norm_state())      # (the observation filter's current vectors)
        return SquashedPolicy(pol, self.action_lo, self.action_hi)

    def state(self, state=None):
        """the learner's state (StepEngine.sac_state's dict), `replay_prio` under prioritised replay and `norm` under running
        normalisers; get or set.  With the ring (sac_buffer) a resumed run continues bit for bit"""
        return history_carry(self.engine,
                             lambda u: self._nstep_state(lambda t: self._norm_carry(lambda s: self._prio_state(self.engine.sac_state, 0, s), 0, t), 0, u), state)

    def load_state(self, state):
        self.state(state)

    def norm_state(self, state=None):
        """the normalisers' state: StepEngine.sac_norm_state's dict plus `returns`, the envs' running discounted returns; get or set"""
        return _norm_state(self.engine, 0, state, family="sac")


class SACPopulationTrainer(PrioritizedReplay, NStepReturns, _NormalizedSAC):
    """M independent SAC learners in lock-step on one engine: member m owns the envs [m n, (m + 1) n), n = N / M, has its own
    actor, twin critics, target critics, temperature, optimiser state, hyperparameters and replay ring, and every launch of a
    store or an update covers all members (StepEngine.sac_pop_*).  What a member computes is bit for bit what SACTrainer computes
    on an engine of its n envs.

    engine: a StepEngine that has been reset; policies: one MLPPolicy (every member starts from it) or a list of M of equal
    shape (2 (K + 1) outputs, log_std_clamp set); configs: one dict of SACTrainer's keyword options (sac()'s keys and
    StepEngine.sac_config's, plus critic_seed and critics) shared by all members, or M of them - M is `members`, or the larger
    of the two counts; action_lo / action_hi [K + 1] (or scalars): the squash bounds, shared by all members.  critic_hidden,
    batch_size, capacity, target_update_interval, learning_starts (transitions of a member's ring), updates_per_iteration and
    n_step (NStepReturns, td3_trainer.py) must be equal in all configurations: the members move together.  prioritized_replay: None, or PrioritizedReplay's dict,
    shared by all members (every member has its own tree).

    normalize_observations / normalize_rewards: every member has its own running normalisers (per_member; _NormalizedSAC above),
    fed from its own envs: member m's are bit for bit a single trainer's of its envs.  norm: dict of obs_min_std, obs_count_cap,
    rew_min_std, rew_count_cap, rew_clip, shared by all members.  state(m) / load_state(m, ...) carry member m's normaliser; a
    PBTScheduler over this trainer copies the donors' normalisers."""

    SHARED = ("critic_hidden", "learning_starts", "updates_per_iteration")

    def __init__(self, engine, policies, configs, action_lo, action_hi, horizon=10, agent_seeds=None, members=None, prioritized_replay=None,
                 normalize_observations=False, normalize_rewards=False, norm=None):
        policies = [policies] if not isinstance(policies, (list, tuple)) else list(policies)
        norm = _norm_options(policies, normalize_observations, normalize_rewards, norm)
        self.normalize_observations, self.normalize_rewards = bool(normalize_observations), bool(normalize_rewards)
        configs = [dict(configs)] if isinstance(configs, dict) else [dict(c) for c in configs]
        n_step = shared_nstep(configs)
        members = max(len(policies), len(configs)) if members is None else int(members)
        if any(len(x) not in (1, members) for x in (policies, configs)) or not policies or not configs:
            raise ValueError("SACPopulationTrainer: policies and configs are each one (shared) or one per member")
        K = policies[0].num_keywords
        A = K + 1
        if any(p.output_size != 2 * A or p.log_std_clamp is None for p in policies):
            raise ValueError("SAC needs policies that end in 2 (K + 1) outputs (means, log-stds) with log_std_clamp set")
        if any(p.shapes() != policies[0].shapes() for p in policies):
            raise ValueError("SACPopulationTrainer: the members' policies must have equal shapes")
        for p in policies[1:]:
            if p.shift is not None and not (np.array_equal(p.shift, policies[0].shift) and np.array_equal(p.scale, policies[0].scale)):
                raise ValueError("SACPopulationTrainer: the normalisation vectors are shared by all members: the policies' must be equal")
        if engine.num_envs % members:
            raise ValueError("the number of members must divide the engine's envs")
        policies, configs = (x if len(x) == members else x * members for x in (policies, configs))
        cfgs = [dict(dict(critic_hidden=(256, 256), learning_starts=1500, updates_per_iteration=64), **c) for c in configs]
        for c in cfgs[1:]:
            if any(tuple(np.atleast_1d(c[k])) != tuple(np.atleast_1d(cfgs[0][k])) for k in self.SHARED):
                raise ValueError("SACPopulationTrainer: critic_hidden, learning_starts and updates_per_iteration must be equal in all configurations")
        hidden = tuple(cfgs[0]["critic_hidden"])
        self.learning_starts, self.updates_per_iteration = int(cfgs[0]["learning_starts"]), int(cfgs[0]["updates_per_iteration"])
        critics, seeds = [c.pop("critics", None) for c in cfgs], [c.pop("critic_seed", m) for m, c in enumerate(cfgs)]
        self.engine, self.members, self.horizon = engine, members, int(horizon)
        self.action_lo, self.action_hi = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32), (A,))) for v in (action_lo, action_hi))
        self._templates = [copy.copy(p) for p in policies]
        self._hidden = hidden
        self.configs = [dict({k: v for k, v in c.items() if k not in self.SHARED}, critic_widths=hidden + (1,)) for c in cfgs]
        engine.mlp_init(self._templates[0], seeds=agent_seeds, deterministic=False)
        engine.mlp_learners(members)
        for m in range(1, members):
            engine.mlp_set_learner(m, self._templates[m])
        engine.mlp_learners_set_squash(self.action_lo, self.action_hi)
        engine.rollout_enable(self.horizon, obs=True)
        engine.sac_pop_init(self.configs)
        for m in range(members):
            engine.sac_pop_set_critics(m, critics[m] if critics[m] is not None else random_critics(K, hidden, seeds[m], policies[0].frames))
        if self._norm_on():
            engine.sac_norm_init(observations=self.normalize_observations, rewards=self.normalize_rewards, per_member=True, **norm)
        self._prio_init(engine, prioritized_replay)
        self._nstep_init(engine, n_step)
        self.history = []

    def iteration(self, days=None, budget=0.0, reset=False, reset_seeds=None):
        """(reset), `days` (default: the horizon) recorded days of run_days("mlp"), the store, and - once every ring holds
        learning_starts transitions - updates_per_iteration updates; returns the M members' statistics, or only the rings' size
        before that"""
        e = self.engine
        if reset:
            e.reset(seeds=reset_seeds)
        e.rollout_reset()
        e.run_days("mlp", self.horizon if days is None else int(days), budget)
        e.sac_pop_store()
        if self._norm_on():
            e.sac_norm_update()             # (one call for all members, whatever their number)
        size = e.sac_pop_buffer(fetch=False)["size"]
        if size >= self.learning_starts:
            self._prio_anneal()
        stats = e.sac_pop_update(self.updates_per_iteration) if size >= self.learning_starts else dict(buffer_size=size, updates=None)
        self.history.append(stats)
        return stats

    def policy(self, member):
        """one member's trained actor with the squash bounds its actions are meant under"""
        pol = policy_from_actor(self._templates[member], self.engine.sac_pop_state(member)["theta"])
        if self.normalize_observations:
            pol = _with_vectors(pol, self.engine.sac_norm_state(member))
        return SquashedPolicy(pol, self.action_lo, self.action_hi)

    def returns(self):
        """[M] float64: per member the mean over its envs of the recorded reward summed over the recorded days"""
        r = self.engine.rollout_fetch()["reward"].astype(np.float64).sum(axis=0)
        return r.reshape(self.members, -1).mean(axis=1)

    def state(self, member, state=None):
        """member's state (StepEngine.sac_pop_state's dict), `replay_prio` under prioritised replay and `norm` under running
        normalisers; get or set"""
        envs = self.engine.num_envs // self.members
        return history_carry(self.engine, lambda w: self._nstep_state(
            lambda u: self._norm_carry(lambda s: self._prio_state(lambda t: self.engine.sac_pop_state(member, t), member, s), member, u, envs), member, w),
            state, member, envs)

    def load_state(self, member, state):
        self.state(member, state)

    def norm_state(self, member, state=None):
        """member's normalisers' state: StepEngine.sac_norm_state's dict plus `returns`, its envs' running discounted returns"""
        return _norm_state(self.engine, member, state, self.engine.num_envs // self.members, family="sac")

    def copy(self, src, dst, with_ring=False):
        """member src's actor, critics, target critics, moments and temperature into member dst (with_ring: its ring too); dst
        keeps its configuration, envs and seed"""
        self.engine.sac_pop_copy(src, dst, with_ring)

    def set_config(self, member, **options):
        """a member's hyperparameters from the next update on: `options` over its current ones (StepEngine.sac_config's; the
        shared fields may not change, init_alpha is not read again)"""
        cfg = dict(self.configs[member], **options)
        self.engine.sac_pop_set_config(member, **cfg)
        self.configs[member] = cfg


__all__ = ["SACPopulationTrainer", "SACTrainer", "SquashedPolicy", "sac"]
