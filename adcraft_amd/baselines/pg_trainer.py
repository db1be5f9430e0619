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

from .mlp_policy import history_carry


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


def rllib_ppo(minibatch_size=None, queued_update=False, **overrides):
    """The PPO configuration of the paper's experiments (RLlib's PPO as the reference's sem_ppo_config sets it), as far as this
    trainer expresses it: gamma 0.995, lambda 0.95, lr 1e-4, clip range 0.5, 20 epochs, and RLlib's loss terms - the adaptive KL
    penalty (kl_coeff 1.0, kl_target 0.01) and the value-loss clip (vf_clip_param 10.0) - through `kl_penalty`.  vf_coef is 2.0
    because our value loss carries a factor 0.5 that RLlib's does not (csrc/adc_pg_kl.h): RLlib's vf_loss_coeff 1.0.
    minibatch_size=64 is the reference's sgd_minibatch_size: minibatches of 64 samples drawn from a new shuffle of the train
    batch every epoch (csrc/adc_pg_shuffle.h) instead of `minibatches` env ranges; without it the preset keeps this trainer's
    own 4 env-range minibatches.  With it RLlib's KL - the mean over the minibatches of an epoch - is what ours is.  What
    remains a configuration choice rather than a difference of the learner: RLlib does not normalise advantages per update
    (normalize_advantages=False) and clips gradients only when asked to (max_grad_norm=0).
    queued_update=True: the trainers run every update as one chain on the device with one host wait (StepEngine.pg_update's
    queued=True) - with 64-sample minibatches an update is hundreds of small steps, and the bits are the same."""
    cfg = ppo(gamma=0.995, lam=0.95, lr=1e-4, eps_clip=0.5, epochs=20, vf_coef=2.0,
              kl_penalty=dict(kl_coef=1.0, kl_target=0.01, adaptive=True, vf_clip=10.0))
    if minibatch_size is not None:
        del cfg["minibatches"]
        cfg["minibatch_size"] = int(minibatch_size)
    if queued_update:
        cfg["queued_update"] = True
    cfg.update(overrides)
    return cfg


_KL_KEYS = {"kl_coef", "kl_target", "adaptive", "vf_clip", "factor_up", "factor_down"}


def _kl_options(kl_penalty, members=None):
    """kl_penalty checked: None, a dict of StepEngine.pg_kl_config's options, or (members given) a list of one dict per member"""
    if kl_penalty is None:
        return None
    many = isinstance(kl_penalty, (list, tuple))
    if many and members is None:
        raise TypeError("kl_penalty: a dict of kl_coef, kl_target, adaptive, vf_clip (a list only for a population)")
    items = list(kl_penalty) if many else [kl_penalty]
    if many and len(items) != members:
        raise ValueError(f"kl_penalty: {len(items)} dicts for {members} members: one dict (shared) or one per member")
    for o in items:
        if not isinstance(o, dict):
            raise TypeError("kl_penalty: a dict of kl_coef, kl_target, adaptive, vf_clip")
        unknown = set(o) - _KL_KEYS
        if unknown:
            raise ValueError(f"kl_penalty: unknown option(s) {sorted(unknown)}: {', '.join(sorted(_KL_KEYS))}")
    return [dict(o) for o in items] if many else dict(items[0])


def _shuffle_options(config, minibatch_size, target_kl, shuffle_seed):
    """(minibatches or None, the add-on's options or None) of a trainer's configuration: minibatch_size takes the role of
    `minibatches`, which then may be left out; giving both is an error"""
    if minibatch_size is not None and "minibatches" in config:
        raise ValueError("minibatches (env ranges) and minibatch_size (shuffled samples) are two ways to cut an update: give one")
    if minibatch_size is None:
        if target_kl is not None or shuffle_seed:
            raise ValueError("target_kl and shuffle_seed belong to shuffled minibatches: give minibatch_size")
        return None
    if int(minibatch_size) < 1:
        raise ValueError("minibatch_size >= 1")
    return dict(minibatch_samples=int(minibatch_size), seed=int(shuffle_seed), target_kl=float(target_kl or 0.0))


def _rew_norm_options(normalize_rewards, rew_norm):
    if rew_norm is not None and not isinstance(rew_norm, dict):
        raise TypeError("rew_norm: a dict of min_std, clip, count_cap")
    if rew_norm and not normalize_rewards:
        raise ValueError("rew_norm given without normalize_rewards=True")
    unknown = set(rew_norm or {}) - {"min_std", "clip", "count_cap"}
    if unknown:
        raise ValueError(f"rew_norm: unknown option(s) {sorted(unknown)}: min_std, clip, count_cap")


def _rew_norm_state(engine, member, state, envs=None):
    """get / set of one normaliser's moments and multiplier together with its envs' running returns (all envs, or the `envs`
    of a member)"""
    sl = slice(None) if envs is None else slice(member * envs, (member + 1) * envs)
    if state is None:
        st = engine.rew_norm_state(member)
        st["returns"] = engine.rew_norm_returns()[sl].copy()
        return st
    engine.rew_norm_state(member, state)
    g = engine.rew_norm_returns()
    g[sl] = np.asarray(state["returns"], dtype=np.float64)
    engine.rew_norm_returns(g)


class PGTrainer:
    """engine: a StepEngine that has been reset; policy: the MLPPolicy to start from (collected stochastically whatever its
    own flag says); horizon: the days of one rollout.  config: ppo() / a2c() or keywords of their kind - `epochs`,
    `minibatches` (must divide the engine's envs) and StepEngine.pg_config's options.  normalize_observations: a running
    mean / std filter of the raw observation on the device (StepEngine.obs_norm_*; the policy must normalise: its shift / scale
    are where the filter starts), updated after every PPO / A2C update; obs_norm: dict(min_std=..., count_cap=...).
    normalize_rewards: the reward in GAE is divided by the running standard deviation of the discounted return, kept on the
    device (StepEngine.rew_norm_*) and updated from every rollout BEFORE its PPO / A2C update; rew_norm: dict(min_std=...,
    clip=..., count_cap=...).  kl_penalty: dict(kl_coef=..., kl_target=..., adaptive=..., vf_clip=...) adds RLlib's analytic KL
    penalty with its adaptive coefficient and the value-loss clip to the loss (StepEngine.pg_kl_*; csrc/adc_pg_kl.h);
    iteration() then also returns `kl`, `kl_coef` (the one the update used) and `vf_clip_fraction`, and state() carries the
    coefficient.  minibatch_size: minibatches of that many samples drawn from a new shuffle of the record every epoch
    (StepEngine.pg_shuffle_*; csrc/adc_pg_shuffle.h) instead of `minibatches` env ranges - give one of the two; target_kl: an
    update ends before the step of the first minibatch whose approx_kl exceeds 1.5 target_kl (Stable-Baselines3's rule);
    shuffle_seed: 0 is the engine's seed.  iteration() then also returns `stopped`, `epochs_begun` and `steps_taken`; the
    order's tick is the optimiser step count, so state() already carries all a resume needs.  queued_update: every update is
    enqueued as one chain with one host wait (StepEngine.pg_update(queued=True)): the same bits, no host round trip per step."""

    def __init__(self, engine, policy, horizon, agent_seeds=None, normalize_observations=False, obs_norm=None, normalize_rewards=False,
                 rew_norm=None, kl_penalty=None, minibatch_size=None, target_kl=None, shuffle_seed=0, queued_update=False, **config):
        _rew_norm_options(normalize_rewards, rew_norm)
        self.queued_update = bool(queued_update)
        self.shuffle = _shuffle_options(config, minibatch_size, target_kl, shuffle_seed)
        cfg = ppo(**config)
        if kl_penalty is None:                  # (a preset carries it among its keys: rllib_ppo())
            kl_penalty = cfg.pop("kl_penalty", None)
        else:
            cfg.pop("kl_penalty", None)
        self.kl_penalty = _kl_options(kl_penalty)
        self.epochs, minibatches = int(cfg.pop("epochs")), int(cfg.pop("minibatches"))
        if self.shuffle is not None:            # (env ranges stay available through StepEngine.pg_minibatch, one env at a time)
            minibatches = engine.num_envs
        if minibatches < 1 or engine.num_envs % minibatches:
            raise ValueError("minibatches must divide the engine's envs")
        self.engine, self._template, self.horizon = engine, policy, int(horizon)
        self.config = dict(cfg, minibatch_envs=engine.num_envs // minibatches)
        engine.mlp_init(policy, seeds=agent_seeds, deterministic=False)
        engine.rollout_enable(self.horizon, obs=True)
        engine.pg_init(**self.config)
        self.normalize_observations = bool(normalize_observations)
        if self.normalize_observations:
            engine.obs_norm_init(**dict(obs_norm or {}))
        self.normalize_rewards = bool(normalize_rewards)
        if self.normalize_rewards:
            engine.rew_norm_init(**dict(rew_norm or {}))
        if self.kl_penalty is not None:
            engine.pg_kl_init(**self.kl_penalty)
        if self.shuffle is not None:
            engine.pg_shuffle_init(**self.shuffle)
        self.history = []

    def iteration(self, days=None, budget=0.0, reset=False, reset_seeds=None):
        """(reset), `days` (default: the horizon) recorded days of run_days("mlp"), the update; returns its statistics.
        budget > 0 overrides the policy's own budget action."""
        e = self.engine
        if reset:
            e.reset(seeds=reset_seeds)
        e.rollout_reset()
        e.run_days("mlp", self.horizon if days is None else int(days), budget)
        if self.normalize_rewards:          # (before the update: this record's rewards are scaled by statistics that include them)
            e.rew_norm_update()
        stats = e.pg_update(self.epochs, queued=True) if self.queued_update else e.pg_update(self.epochs)
        if self.kl_penalty is not None:
            kl = e.pg_kl_stats()
            stats.update(kl=kl["kl"], kl_coef=kl["kl_coef"], vf_clip_fraction=kl["vf_clip_fraction"])
        if self.shuffle is not None:
            sh = e.pg_shuffle_stats()
            stats.update(stopped=bool(sh["stopped"]), epochs_begun=sh["epochs_begun"], steps_taken=sh["steps_taken"])
        if self.normalize_observations:     # (after the update: its bootstrap value is evaluated under the vectors of the record)
            e.obs_norm_update()
        self.history.append(stats)
        return stats

    def policy(self):
        """an MLPPolicy holding the trained policy layers, value layers and log_std (and, with normalize_observations, the
        filter's current shift and scale: it evaluates as the trainer's does)"""
        out = policy_from_flat(self._template, self.engine.pg_state()["theta"])
        if self.normalize_observations:
            st = self.engine.obs_norm_state()
            out.shift, out.scale = st["shift"], st["scale"]
        return out

    def obs_norm_state(self, state=None):
        """the filter's state (StepEngine.obs_norm_state); with state() a run resumes bit for bit"""
        return self.engine.obs_norm_state(0, state)

    def rew_norm_state(self, state=None):
        """the reward normaliser's state: StepEngine.rew_norm_state's dict plus `returns`, the envs' running discounted returns
        [N]; with state() a run resumes bit for bit"""
        return _rew_norm_state(self.engine, 0, state)

    def state(self, state=None):
        """the trainer's state (StepEngine.pg_state's dict; with kl_penalty also `kl_coef`, with MLPPolicy(frames > 1) also
        `obs_history`); set: the run continues bit for bit"""
        return history_carry(self.engine, self._state, state)

    def load_state(self, state):
        self.state(state)

    def _state(self, state):
        if state is None:
            st = self.engine.pg_state()
            if self.kl_penalty is not None:
                st["kl_coef"] = self.engine.pg_kl_coef(0)
            return st
        self.engine.pg_state(state)
        if self.kl_penalty is not None and "kl_coef" in state:
            self.engine.pg_kl_coef(0, state["kl_coef"])


class PGPopulationTrainer:
    """M independent PPO / A2C learners in lock-step on one engine: member m owns the envs [m n, (m + 1) n), n = N / M, has its
    own policy network, value network, log_std, optimiser state and hyperparameters, and every launch of an update covers all
    members (StepEngine.pg_pop_*).  What a member computes is bit for bit what PGTrainer computes on an engine of its n envs.

    engine: a StepEngine that has been reset; policies: one MLPPolicy (every member starts from it) or M of equal shape - M is
    then the number of configs, or of policies; configs: one dict of ppo() / a2c() kind shared by all members or M of them;
    `epochs` and `minibatches` (of a member's envs) must be equal in all of them.  agent_seeds: [N] as PGTrainer's.
    normalize_observations: one running observation filter PER MEMBER, fed from the member's own envs (the members' policies
    may then carry different shift / scale: each member starts from its own); obs_norm: dict(min_std=..., count_cap=...).
    normalize_rewards: one running reward normaliser PER MEMBER (PGTrainer's), fed from the member's own envs under the
    member's own gamma; rew_norm: dict(min_std=..., clip=..., count_cap=...).  kl_penalty: PGTrainer's dict shared by all
    members, or a list of one per member; every member has its own coefficient that adapts on its own either way.
    `minibatch_size` (equal in all members, instead of `minibatches`), `target_kl` and `shuffle_seed` in the members'
    configurations: PGTrainer's shuffled minibatches, every member with its own seed and stopping on its own while the others
    go on.  queued_update (or `queued_update` in the members' configurations, as rllib_ppo(queued_update=True) carries it): every
    update is enqueued as one chain with one host wait (StepEngine.pg_pop_update(queued=True)): the same bits."""

    def __init__(self, engine, policies, horizon, configs, agent_seeds=None, normalize_observations=False, obs_norm=None, normalize_rewards=False,
                 rew_norm=None, kl_penalty=None, queued_update=False):
        _rew_norm_options(normalize_rewards, rew_norm)
        policies = [policies] if not isinstance(policies, (list, tuple)) else list(policies)
        configs = [configs] if isinstance(configs, dict) else list(configs)
        self.queued_update = bool(queued_update) or any(c.get("queued_update") for c in configs)      # (one chain covers all members)
        configs = [{k: v for k, v in c.items() if k != "queued_update"} for c in configs]
        if not policies or not configs:
            raise ValueError("PGPopulationTrainer: at least one policy and one configuration")
        members = max(len(policies), len(configs))
        if len(policies) not in (1, members) or len(configs) not in (1, members):
            raise ValueError(f"PGPopulationTrainer: {len(policies)} policies and {len(configs)} configurations: each is one (shared) or one per member")
        if any(p.shapes() != policies[0].shapes() for p in policies):
            raise ValueError("PGPopulationTrainer: the members' policies must have equal shapes (layers, value layers, free log_std, normalisation)")
        self.normalize_observations = bool(normalize_observations)
        for p in policies[1:]:
            if self.normalize_observations:
                break
            if p.shift is not None and not (np.array_equal(p.shift, policies[0].shift) and np.array_equal(p.scale, policies[0].scale)):
                raise ValueError("PGPopulationTrainer: the normalisation vectors are shared by all members: the policies' must be equal")
        shuffles = [_shuffle_options(c, c.get("minibatch_size"), c.get("target_kl"), c.get("shuffle_seed", 0)) for c in configs]
        if any(s is None for s in shuffles) and any(s is not None for s in shuffles):
            raise ValueError("PGPopulationTrainer: minibatch_size in some members' configurations and not in others")
        self.shuffle = None if shuffles[0] is None else shuffles
        if self.shuffle is not None and len({s["minibatch_samples"] for s in shuffles}) != 1:
            raise ValueError("PGPopulationTrainer: minibatch_size must be equal in all members' configurations (the members move in lock-step)")
        cfgs = [ppo(**{k: v for k, v in c.items() if k not in ("minibatch_size", "target_kl", "shuffle_seed")}) for c in configs]
        preset = [c.pop("kl_penalty", None) for c in cfgs]             # (a preset carries it among its keys: rllib_ppo())
        if kl_penalty is None and any(p is not None for p in preset):
            if any(p is None for p in preset):
                raise ValueError("PGPopulationTrainer: kl_penalty in some members' configurations and not in others")
            kl_penalty = preset if len(preset) == members else preset[0]
        self.kl_penalty = _kl_options(kl_penalty, members)
        self.epochs, minibatches = int(cfgs[0].pop("epochs")), int(cfgs[0].pop("minibatches"))
        for c in cfgs[1:]:
            if (int(c.pop("epochs")), int(c.pop("minibatches"))) != (self.epochs, minibatches):
                raise ValueError("PGPopulationTrainer: epochs and minibatches must be equal in all members' configurations (the members move in lock-step)")
        if members < 1 or engine.num_envs % members:
            raise ValueError("the number of members must divide the engine's envs")
        n = engine.num_envs // members
        if self.shuffle is not None:
            minibatches = n
        if minibatches < 1 or n % minibatches:
            raise ValueError("minibatches must divide the envs of a member")
        self.engine, self.members, self.horizon = engine, members, int(horizon)
        self._templates = policies if len(policies) == members else policies * members
        self.configs = [dict(c, minibatch_envs=n // minibatches) for c in cfgs]
        engine.mlp_init(policies[0], seeds=agent_seeds, deterministic=False)
        engine.mlp_learners(members)
        if len(policies) > 1:
            for m, pol in enumerate(policies):
                engine.mlp_set_learner(m, pol)
        engine.rollout_enable(self.horizon, obs=True)
        engine.pg_pop_init(self.configs)
        if self.normalize_observations:
            engine.obs_norm_init(per_member=True, **dict(obs_norm or {}))
            if len(policies) > 1:
                for m, pol in enumerate(policies):
                    st = engine.obs_norm_state(m)
                    st["shift"], st["scale"] = pol.shift, pol.scale
                    engine.obs_norm_state(m, st)
        self.normalize_rewards = bool(normalize_rewards)
        if self.normalize_rewards:
            engine.rew_norm_init(per_member=True, **dict(rew_norm or {}))
        if isinstance(self.kl_penalty, list):
            engine.pg_kl_init(per_member=self.kl_penalty)
        elif self.kl_penalty is not None:
            engine.pg_kl_init(**self.kl_penalty)
        if self.shuffle is not None:
            engine.pg_shuffle_init(per_member=self.shuffle * (members if len(self.shuffle) == 1 else 1))
        self.history = []

    def iteration(self, days=None, budget=0.0, reset=False, reset_seeds=None):
        """(reset), `days` (default: the horizon) recorded days of run_days("mlp"), the update; returns the M members' statistics"""
        e = self.engine
        if reset:
            e.reset(seeds=reset_seeds)
        e.rollout_reset()
        e.run_days("mlp", self.horizon if days is None else int(days), budget)
        if self.normalize_rewards:
            e.rew_norm_update()
        stats = e.pg_pop_update(self.epochs, queued=True) if self.queued_update else e.pg_pop_update(self.epochs)
        if self.kl_penalty is not None:
            for st, kl in zip(stats, e.pg_kl_stats()):
                st.update(kl=kl["kl"], kl_coef=kl["kl_coef"], vf_clip_fraction=kl["vf_clip_fraction"])
        if self.shuffle is not None:
            for st, sh in zip(stats, e.pg_shuffle_stats()):
                st.update(stopped=bool(sh["stopped"]), epochs_begun=sh["epochs_begun"], steps_taken=sh["steps_taken"])
        if self.normalize_observations:
            e.obs_norm_update()
        self.history.append(stats)
        return stats

    def policy(self, member):
        """an MLPPolicy holding one member's trained policy layers, value layers and log_std (and, with normalize_observations,
        the member's filter's current shift and scale)"""
        out = policy_from_flat(self._templates[member], self.engine.pg_pop_state(member)["theta"])
        if self.normalize_observations:
            st = self.engine.obs_norm_state(member)
            out.shift, out.scale = st["shift"], st["scale"]
        return out

    def obs_norm_state(self, member, state=None):
        return self.engine.obs_norm_state(member, state)

    def rew_norm_state(self, member, state=None):
        """member's reward normaliser (PGTrainer.rew_norm_state's dict; `returns` holds the member's own envs')"""
        return _rew_norm_state(self.engine, member, state, self.engine.num_envs // self.members)

    def returns(self):
        """[M] float64: per member the mean over its envs of the recorded reward summed over the recorded days (from the
        record's reward array alone)"""
        r = self.engine.rollout_fetch()["reward"].astype(np.float64).sum(axis=0)
        return r.reshape(self.members, -1).mean(axis=1)

    def state(self, member, state=None):
        """one member's state (StepEngine.pg_pop_state's dict; with kl_penalty also `kl_coef`, with MLPPolicy(frames > 1) also
        `obs_history`, its own envs')"""
        return history_carry(self.engine, lambda s: self._state(member, s), state, member, self.engine.num_envs // self.members)

    def load_state(self, member, state):
        self.state(member, state)

    def _state(self, member, state):
        if state is None:
            st = self.engine.pg_pop_state(member)
            if self.kl_penalty is not None:
                st["kl_coef"] = self.engine.pg_kl_coef(member)
            return st
        self.engine.pg_pop_state(member, state)
        if self.kl_penalty is not None and "kl_coef" in state:
            self.engine.pg_kl_coef(member, state["kl_coef"])


__all__ = ["PGPopulationTrainer", "PGTrainer", "ppo", "a2c", "rllib_ppo", "flat_params", "policy_from_flat"]
