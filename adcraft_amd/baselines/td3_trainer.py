"""TD3 (Fujimoto, van Hoof, Meger 2018, "Addressing Function Approximation Error in Actor-Critic Methods") for the
device-resident MLP policy: the deterministic policy gradient (Lillicrap et al. 2016) with twin critics, clipped target
smoothing noise and delayed actor / target updates, over a replay ring that lives on the device.  `run_days("mlp")` records the
rollout, `td3_store` appends it to the ring, `td3_update` samples minibatches, trains the critics and - every policy_delay-th
update - the actor, and writes the new actor where the next day's policy kernel reads it: collect -> store -> update runs
without a transition leaving HBM.  The arithmetic is csrc/adc_td3.h; StepEngine.td3_* are the calls.

The actor is the MLPPolicy's policy network with the free log_std head; its mean is the deterministic action and
mean + exp(log_std) * z, log_std = log(exploration sigma), the exploration.  The reference's pure-random warm-up
(`random_timesteps`) is covered by collecting under the initial policy with a larger sigma for the first iterations:
`TD3Trainer.set_exploration(sigma)`, then back.  n_step > 1 turns on n-step returns (StepEngine.replay_nstep_*; the law is
csrc/adc_td3.h "n-step") for the trainer's ring(s).

action_bounds=(lo, hi) turns on the bounded mode (csrc/adc_mlp.h "bounded", csrc/adc_td3.h "bounded"), the way RLlib's DDPG
family and Stable-Baselines3 run TD3: the actor is tanh-squashed into the action box, the exploration noise is added to the
squashed action and clipped to the box, the ring and the critics hold the action in units of the box, and the first
random_timesteps transitions are collected with actions drawn uniformly from the box.  rllib_td3(lo, hi) is the paper's
`sem_td3_config` in these terms."""
import copy

import numpy as np

from .mlp_policy import history_carry


def td3(**overrides):
    """Fujimoto et al.'s configuration: gamma 0.99, tau 0.005, actor and targets every 2nd update, target noise 0.2 clipped at
    0.5, batches of 256, both learning rates 1e-3, exploration sigma 0.1, critics of two hidden layers of 256"""
    cfg = dict(critic_hidden=(256, 256), exploration_sigma=0.1, learning_starts=10000, updates_per_iteration=64, gamma=0.99, tau=0.005,
               policy_delay=2, target_noise=0.2, target_noise_clip=0.5, batch_size=256, capacity=1000000, actor_lr=1e-3, critic_lr=1e-3,
               optimiser="adam")
    cfg.update(overrides)
    return cfg


def rllib_td3(lo, hi, **overrides):
    """TD3Trainer's keyword options for the paper's `sem_td3_config` (RLlib's TD3Config) as far as this trainer expresses it, on
    the action box [lo, hi] (scalars, or [K + 1] in the flat action order; the reference's own action space has no finite upper
    bound, so the box is the user's): gamma 0.995, both learning rates 1e-3, batches of 2048, tau 0.005, a ring of 1e6,
    random_timesteps = learning_starts = 10000, policy_delay 2 and target noise 0.2 clipped at 0.5 (RLlib's TD3 defaults), and
    RLlib's Gaussian exploration of stddev 0.1 in action units converted to units of the half-range (sigma = 0.1 / (0.5 (hi - lo)):
    about 0.067 on [0.01, 3]; the bounds must then have one width, or give exploration_sigma yourself).  The critics are
    (256, 256) where the paper has fcnet_hiddens [400, 300]: hidden widths above 256 are not supported.  The paper's relu
    activation is the MLPPolicy's to choose."""
    half = np.unique(0.5 * (np.asarray(hi, np.float64) - np.asarray(lo, np.float64)))
    cfg = dict(action_bounds=(lo, hi), critic_hidden=(256, 256), learning_starts=10000, random_timesteps=10000, gamma=0.995, tau=0.005,
               policy_delay=2, target_noise=0.2, target_noise_clip=0.5, batch_size=2048, capacity=1000000, actor_lr=1e-3, critic_lr=1e-3,
               optimiser="adam")
    if "exploration_sigma" not in overrides:
        if half.size != 1 or not half[0] > 0.0:
            raise ValueError("rllib_td3: the bounds' widths differ (or are not positive): give exploration_sigma in units of the half-range")
        cfg["exploration_sigma"] = 0.1 / float(half[0])
    cfg.update(overrides)
    return cfg


def action_box(action_bounds, K):
    """(lo, hi) float32 [K + 1] from action_bounds = (lo, hi), scalars or vectors in the flat action order; None stays None"""
    if action_bounds is None:
        return None
    if len(action_bounds) != 2:
        raise ValueError("action_bounds: a pair (lo, hi)")
    lo, hi = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float32), (K + 1,))).copy() for v in action_bounds)
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(hi > lo)):
        raise ValueError("action_bounds: finite, hi > lo")
    return lo, hi


class BoundedActions:
    """the trainers' side of action_bounds / random_timesteps.  Under bounds exploration_sigma is one scalar in units of the
    half-range 0.5 (hi - lo) - RLlib's 0.1 dollars on a [0.01, 3] box is about 0.067 - so set_exploration and the PBT scheduler's
    sigma perturbation work unchanged.  An iteration collects in the act's random mode while fewer than random_timesteps
    transitions have been stored in (a member's) ring, and in the gaussian mode from then on.  A trainer's state() carries
    `bounded` - the bounds, the mode and random_timesteps - and refuses a state made under other bounds."""

    def _bounds_check(self, action_bounds, random_timesteps, K, action_norms):
        self.action_bounds = action_box(action_bounds, K)
        if isinstance(random_timesteps, bool) or int(random_timesteps) != random_timesteps or int(random_timesteps) < 0:
            raise ValueError("random_timesteps: an integer >= 0")
        self.random_timesteps = int(random_timesteps)
        if self.random_timesteps and self.action_bounds is None:
            raise ValueError("random_timesteps needs action_bounds: the warm-up's actions are drawn uniformly from the box")
        if self.action_bounds is not None and any(n is not None for n in action_norms):
            raise ValueError("action_bounds with action_norm is not supported: the critics read the action in [-1, 1] as stored")

    def _explore_for(self, written):
        """before a collection: the act's mode from the transitions stored so far"""
        if self.action_bounds is not None:
            self.engine.mlp_set_explore("random" if written < self.random_timesteps else "gaussian")

    def _bounded_state(self, get_or_set, state):
        if state is None:
            st = get_or_set(None)
            if self.action_bounds is not None:
                st["bounded"] = dict(lo=self.action_bounds[0].copy(), hi=self.action_bounds[1].copy(), explore=self.engine.mlp_bounds()["explore"],
                                     random_timesteps=self.random_timesteps)
            return st
        state = dict(state)
        b = state.pop("bounded", None)
        if (b is None) != (self.action_bounds is None):
            raise ValueError("the state was made " + ("without" if b is None else "under") + " action_bounds, and this trainer was not")
        if b is not None:
            if not (np.array_equal(b["lo"], self.action_bounds[0]) and np.array_equal(b["hi"], self.action_bounds[1])):
                raise ValueError("the state was made under other action_bounds: its ring's actions are in units of those")
            self.random_timesteps = int(b["random_timesteps"])
        get_or_set(state)
        if b is not None:
            self.engine.mlp_set_explore(b["explore"])

    def _squashed(self, pol):
        """the exported policy: under bounds with the box its actions are meant under (a deterministic act of it through
        mlp_set_squash gives the env the bits the bounded act gives it)"""
        if self.action_bounds is None:
            return pol
        from .sac_trainer import SquashedPolicy
        return SquashedPolicy(pol, *self.action_bounds)


def random_critics(K, hidden, seed=0, frames=1):
    """two critics on the frames (5K + 2) + K + 1 inputs [x | action] with torch's default Linear initialisation: weights and
    biases uniform in +- 1 / sqrt(n_in)"""
    rng, out = np.random.default_rng(seed), []
    for _ in range(2):
        layers, n_in = [], int(frames) * (5 * K + 2) + K + 1
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


NORM_OPTIONS = ("obs_min_std", "obs_count_cap", "rew_min_std", "rew_count_cap", "rew_clip")


def _norm_options(policies, normalize_observations, normalize_rewards, norm):
    """the checks on the normalisers' arguments that need no device"""
    if norm is not None and not isinstance(norm, dict):
        raise TypeError("norm: a dict of " + ", ".join(NORM_OPTIONS))
    if norm and not (normalize_observations or normalize_rewards):
        raise ValueError("norm given without normalize_observations=True or normalize_rewards=True")
    unknown = set(norm or {}) - set(NORM_OPTIONS)
    if unknown:
        raise ValueError(f"norm: unknown option(s) {sorted(unknown)}: " + ", ".join(NORM_OPTIONS))
    if normalize_observations and any(p.shift is None for p in policies):
        raise ValueError("normalize_observations needs a policy with normalisation vectors (shift / scale): they are the filter's start")
    return dict(norm or {})


def _with_vectors(policy, state):
    """`policy` with the observation filter's current vectors"""
    if "shift" in state:
        policy.shift, policy.scale = state["shift"].copy(), state["scale"].copy()
    return policy


def _norm_state(engine, member, state, envs=None, family="td3"):
    """StepEngine.td3_norm_state's dict (family "sac": sac_norm_state's) plus `returns`, the (member's) envs' running discounted
    returns, when rewards are normalised"""
    norm_state, norm_returns = getattr(engine, family + "_norm_state"), getattr(engine, family + "_norm_returns")
    n = engine.num_envs if envs is None else envs
    sl = slice(0, n) if envs is None else slice(member * n, (member + 1) * n)
    if state is None:
        st = norm_state(member)
        if "rew_count" in st:
            st["returns"] = norm_returns()[sl].copy()
        return st
    norm_state(member, state)
    if "returns" in state:
        g = norm_returns()
        g[sl] = state["returns"]
        norm_returns(g)


class PrioritizedReplay:
    """the trainers' side of prioritized_replay=None | dict(alpha=0.6, beta=0.4, eps=1e-6, cap=1e6, beta_final=None,
    beta_iterations=0): prioritised replay on the device (StepEngine.replay_prio_*; csrc/adc_per.h) for the trainer's ring(s).
    With beta_final and beta_iterations > 0 the importance weights' exponent moves linearly from beta to beta_final over that
    many iterations, set on the host before an iteration's updates.  A trainer's state() then carries `replay_prio` - the leaves,
    top and the iteration count - and, set after the ring was loaded, a resumed run continues bit for bit.  What prioritisation
    gains in learning on this env has not been measured."""

    PRIO_DEFAULTS = dict(alpha=0.6, beta=0.4, eps=1e-6, cap=1e6, beta_final=None, beta_iterations=0)

    def _prio_init(self, engine, prioritized_replay):
        self.prioritized_replay, self._prio_iterations = None, 0
        if prioritized_replay is None:
            return
        unknown = set(prioritized_replay) - set(self.PRIO_DEFAULTS)
        if unknown:
            raise ValueError(f"prioritized_replay: unknown keys {sorted(unknown)}")
        o = dict(self.PRIO_DEFAULTS, **prioritized_replay)
        if o["beta_final"] is not None and not 0.0 <= float(o["beta_final"]) <= 1.0:
            raise ValueError("prioritized_replay: beta_final must be in [0, 1]")
        engine.replay_prio_init(alpha=o["alpha"], beta=o["beta"], eps=o["eps"], cap=o["cap"])
        self.prioritized_replay = o

    def _prio_anneal(self):
        """before an iteration's updates: iteration i of the run uses beta + min(i / beta_iterations, 1) (beta_final - beta)"""
        o = self.prioritized_replay
        if o is None:
            return
        if o["beta_final"] is not None and int(o["beta_iterations"]) > 0:
            f = min(self._prio_iterations / float(o["beta_iterations"]), 1.0)
            self.engine.replay_prio_set_beta(float(o["beta"]) + f * (float(o["beta_final"]) - float(o["beta"])))
        self._prio_iterations += 1

    def _prio_state(self, get_or_set, member, state):
        """get_or_set(state): the engine's own state call; `replay_prio` rides along"""
        if state is None:
            st = get_or_set(None)
            if self.prioritized_replay is not None:
                st["replay_prio"] = dict(self.engine.replay_prio_state(member), iterations=self._prio_iterations)
            return st
        state = dict(state)
        prio = state.pop("replay_prio", None)
        get_or_set(state)
        if prio is not None and self.prioritized_replay is not None:
            self.engine.replay_prio_state(member, prio)
            self._prio_iterations = int(prio.get("iterations", self._prio_iterations))


def nstep_check(n_step):
    """n_step as an int in 1..16 (the engine's own refusal, which needs no device)"""
    import ctypes

    from .. import _ffi
    if isinstance(n_step, bool) or int(n_step) != n_step:
        raise ValueError("n_step: an integer from 1 to 16")
    msg = ctypes.c_char_p()
    if _ffi.lib().adc_replay_nstep_check(int(n_step), ctypes.byref(msg)) != _ffi.ADC_OK:
        raise ValueError("n_step: " + (msg.value or b"1 to 16").decode())
    return int(n_step)


def shared_nstep(configs):
    """n_step of a population's configurations (taken out of them): a shared key, refused when it differs"""
    steps = [c.pop("n_step", 1) for c in configs]
    if any(n != steps[0] for n in steps):
        raise ValueError("n_step is shared by all members (one window for every ring): it must be equal in all configurations")
    return nstep_check(steps[0])


class NStepReturns:
    """the trainers' side of n_step: with n_step > 1 the store writes n-step returns and the targets bootstrap with the slots' own
    discounts (StepEngine.replay_nstep_*; csrc/adc_td3.h "n-step"); with n_step == 1 the add-on is never initialised and every call
    launches what it launched.  A trainer's state() then carries `replay_nstep` - n and the slots' gn - set after the ring was
    loaded.  What n-step returns gain in learning on this env has not been measured."""

    def _nstep_init(self, engine, n_step):
        self.n_step = nstep_check(n_step)
        if self.n_step > 1:
            engine.replay_nstep_init(self.n_step)

    def _nstep_state(self, get_or_set, member, state):
        """get_or_set(state): the trainer's own state call; `replay_nstep` rides along"""
        if state is None:
            st = get_or_set(None)
            if self.n_step > 1:
                st["replay_nstep"] = self.engine.replay_nstep_state(member)
            return st
        state = dict(state)
        nstep = state.pop("replay_nstep", None)
        get_or_set(state)
        if nstep is not None and self.n_step > 1:
            self.engine.replay_nstep_state(member, nstep)


class TD3Trainer(PrioritizedReplay, NStepReturns, BoundedActions):
    """engine: a StepEngine that has been reset; policy: the MLPPolicy to start from (K + 1 means, free log_std; a value network
    is ignored); critic_hidden: the critics' hidden widths (each <= 256); horizon: the days of one collection;
    exploration_sigma: the standard deviation of the collection noise; learning_starts: transitions the ring must hold before
    the first update; updates_per_iteration: critic updates after every collection.  config: td3()'s other keys and
    StepEngine.td3_config's options, plus critic_seed (random_critics' seed), critics (two lists of layers, instead) and
    action_norm ((shift, scale) [K + 1] for the critics' action inputs).

    normalize_observations / normalize_rewards: running normalisers on the device (StepEngine.td3_norm_*; csrc/adc_td3_norm.h).
    The record and the ring then hold raw observations and raw rewards and every batch is normalised as it is sampled, with the
    statistics updated from every collection BEFORE its updates; norm: dict(obs_min_std=..., obs_count_cap=..., rew_min_std=...,
    rew_count_cap=..., rew_clip=...).  What they gain in learning has not been measured.

    prioritized_replay: None, or PrioritizedReplay's dict.  n_step: the window of n-step returns, 1 (off) to 16 (NStepReturns).

    action_bounds: None, or (lo, hi) - scalars or [K + 1] in the flat action order (budget, bids): the bounded mode
    (BoundedActions).  exploration_sigma is then in units of the half-range 0.5 (hi - lo), one scalar: RLlib's 0.1 dollars on a
    [0.01, 3] box is about 0.067; target_noise and target_noise_clip are in those units too, as Fujimoto's 0.2 / 0.5 are.
    action_lo / action_hi and action_norm are refused with it.  random_timesteps: the transitions collected with actions drawn
    uniformly from the box before the Gaussian exploration starts (RLlib's exploration_config).  policy() then returns
    sac_trainer's SquashedPolicy (the actor and its bounds)."""

    def __init__(self, engine, policy, critic_hidden=(256, 256), horizon=10, exploration_sigma=0.1, learning_starts=10000, updates_per_iteration=64,
                 agent_seeds=None, normalize_observations=False, normalize_rewards=False, norm=None, prioritized_replay=None, n_step=1,
                 action_bounds=None, random_timesteps=0, **config):
        norm = _norm_options([policy], normalize_observations, normalize_rewards, norm)
        n_step = nstep_check(n_step)
        if policy.log_std is None:
            raise ValueError("TD3 needs a policy that ends in K + 1 means with the free log_std vector")
        self.normalize_observations, self.normalize_rewards = bool(normalize_observations), bool(normalize_rewards)
        cfg = dict(config)
        critics, action_norm = cfg.pop("critics", None), cfg.pop("action_norm", None)
        critic_seed = cfg.pop("critic_seed", 0)
        self._bounds_check(action_bounds, random_timesteps, policy.num_keywords, [action_norm])
        self.engine, self.horizon = engine, int(horizon)
        self.learning_starts, self.updates_per_iteration = int(learning_starts), int(updates_per_iteration)
        self._template = copy.copy(policy)
        self._template.log_std = np.full(policy.num_keywords + 1, np.log(exploration_sigma), np.float32)
        self.config = dict(cfg, critic_widths=tuple(critic_hidden) + (1,))
        engine.mlp_init(self._template, seeds=agent_seeds, deterministic=False)
        if self.action_bounds is not None:
            engine.mlp_set_bounds(*self.action_bounds)
        engine.rollout_enable(self.horizon, obs=True)
        engine.td3_init(**self.config)
        engine.td3_set_critics(critics if critics is not None else random_critics(policy.num_keywords, critic_hidden, critic_seed, policy.frames), action_norm=action_norm)
        if self.action_bounds is not None:
            engine.td3_set_bounded(True)
        if self.normalize_observations or self.normalize_rewards:
            engine.td3_norm_init(observations=self.normalize_observations, rewards=self.normalize_rewards, **norm)
        self._prio_init(engine, prioritized_replay)
        self._nstep_init(engine, n_step)
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
        if self.action_bounds is not None:
            self._explore_for(e.td3_buffer(fetch=False)["written"])
        e.run_days("mlp", self.horizon if days is None else int(days), budget)
        e.td3_store()
        if self.normalize_observations or self.normalize_rewards:
            e.td3_norm_update()             # (the batches below are scaled by statistics that include the newest days)
        size = e.td3_buffer(fetch=False)["size"]
        if size >= self.learning_starts:
            self._prio_anneal()
        stats = e.td3_update(self.updates_per_iteration) if size >= self.learning_starts else dict(buffer_size=size, updates=None)
        self.history.append(stats)
        return stats

    def demonstrate(self, teacher, days=None, budget=0.0):
        """`days` (default: the horizon) teacher days (StepEngine.teach_days) into the ring: the expert's transitions before
        learning starts (RLlib's configuration spends random_timesteps on uniform noise there: action_bounds with
        random_timesteps does that).  teacher: "oracle", "interpolation", "zero_margin" or "fixed"; the engine must hold what that
        teacher needs.  Under action_bounds the ring holds the teacher's actions in units of the box, clipped to it.  Returns the
        ring's size."""
        e = self.engine
        e.rollout_reset()
        e.teach_days(teacher, self.horizon if days is None else int(days), budget)
        e.td3_store()
        if self.normalize_observations or self.normalize_rewards:
            e.td3_norm_update()
        return e.td3_buffer(fetch=False)["size"]

    def policy(self):
        """an MLPPolicy holding the trained actor (its log_std the exploration's; under a running observation normaliser its
        shift / scale are the current vectors)"""
        pol = policy_from_actor(self._template, self.engine.td3_state()["theta"])
        return self._squashed(_with_vectors(pol, self.engine.td3_norm_state()) if self.normalize_observations else pol)

    def state(self, state=None):
        """the learner's state (StepEngine.td3_state's dict), `replay_prio` under prioritised replay, `replay_nstep` under n-step
        returns and `obs_history` with MLPPolicy(frames > 1); get or set"""
        return history_carry(self.engine,
                             lambda u: self._bounded_state(lambda t: self._nstep_state(lambda s: self._prio_state(self.engine.td3_state, 0, s), 0, t), u), state)

    def load_state(self, state):
        self.state(state)

    def norm_state(self, state=None):
        """the normalisers' state: StepEngine.td3_norm_state's dict plus `returns`, the envs' running discounted returns; get or set"""
        return _norm_state(self.engine, 0, state)


class TD3PopulationTrainer(PrioritizedReplay, NStepReturns, BoundedActions):
    """M independent TD3 learners in lock-step on one engine: member m owns the envs [m n, (m + 1) n), n = N / M, has its own
    actor, exploration sigma, twin critics, targets, optimiser state, hyperparameters and replay ring, and every launch of a
    store or an update covers all members (StepEngine.td3_pop_*).  What a member computes is bit for bit what TD3Trainer
    computes on an engine of its n envs.

    engine: a StepEngine that has been reset; policies: one MLPPolicy (every member starts from it) or M of equal shape;
    sigmas: one exploration sigma or M, or None: every configuration's exploration_sigma (default 0.1); configs: one dict of
    TD3Trainer's keyword options (td3()'s keys and StepEngine.td3_config's, plus critic_seed, critics, action_norm) shared by
    all members or M of them - M is `members`, or the largest of the three counts.  critic_hidden, batch_size, capacity, policy_delay, learning_starts (transitions of a member's ring),
    updates_per_iteration, n_step and action_norm must be equal in all configurations: the members move together.

    normalize_observations / normalize_rewards: every member has its own running normalisers (TD3Trainer's, per member: a
    member's statistics are bit for bit a single trainer's of its envs; the reward's discount is the member's own gamma); norm as
    TD3Trainer's.  prioritized_replay: None, or PrioritizedReplay's dict, shared by all members (every member has its own tree).

    action_bounds / random_timesteps: TD3Trainer's, one pair of bounds shared by all members; the sigmas are then in units of the
    half-range.  The members' rings fill together, so the warm-up ends for all at once."""

    SHARED = ("critic_hidden", "learning_starts", "updates_per_iteration")

    def __init__(self, engine, policies, sigmas, configs, horizon=10, agent_seeds=None, members=None, normalize_observations=False,
                 normalize_rewards=False, norm=None, prioritized_replay=None, action_bounds=None, random_timesteps=0):
        policies = [policies] if not isinstance(policies, (list, tuple)) else list(policies)
        norm = _norm_options(policies, normalize_observations, normalize_rewards, norm)
        self.normalize_observations, self.normalize_rewards = bool(normalize_observations), bool(normalize_rewards)
        configs = [dict(configs)] if isinstance(configs, dict) else [dict(c) for c in configs]
        n_step = shared_nstep(configs)
        own = [c.pop("exploration_sigma", 0.1) for c in configs]
        sigmas = own if sigmas is None else [float(sigmas)] if np.isscalar(sigmas) else [float(s) for s in sigmas]
        members = max(len(policies), len(sigmas), len(configs)) if members is None else int(members)
        if any(len(x) not in (1, members) for x in (policies, sigmas, configs)) or not policies or not sigmas or not configs:
            raise ValueError("TD3PopulationTrainer: policies, sigmas and configs are each one (shared) or one per member")
        if any(p.log_std is None for p in policies):
            raise ValueError("TD3 needs policies that end in K + 1 means with the free log_std vector")
        if any(p.shapes() != policies[0].shapes() for p in policies):
            raise ValueError("TD3PopulationTrainer: the members' policies must have equal shapes")
        for p in policies[1:]:
            if p.shift is not None and not (np.array_equal(p.shift, policies[0].shift) and np.array_equal(p.scale, policies[0].scale)):
                raise ValueError("TD3PopulationTrainer: the normalisation vectors are shared by all members: the policies' must be equal")
        if engine.num_envs % members:
            raise ValueError("the number of members must divide the engine's envs")
        policies, sigmas, configs = (x if len(x) == members else x * members for x in (policies, sigmas, configs))
        K = policies[0].num_keywords
        cfgs = [dict(dict(critic_hidden=(256, 256), learning_starts=10000, updates_per_iteration=64), **c) for c in configs]
        for c in cfgs[1:]:
            if any(tuple(np.atleast_1d(c[k])) != tuple(np.atleast_1d(cfgs[0][k])) for k in self.SHARED):
                raise ValueError("TD3PopulationTrainer: critic_hidden, learning_starts and updates_per_iteration must be equal in all configurations")
        hidden = tuple(cfgs[0]["critic_hidden"])
        self.learning_starts, self.updates_per_iteration = int(cfgs[0]["learning_starts"]), int(cfgs[0]["updates_per_iteration"])
        critics, norms, seeds = [c.pop("critics", None) for c in cfgs], [c.pop("action_norm", None) for c in cfgs], [c.pop("critic_seed", m) for m, c in enumerate(cfgs)]
        for n in norms[1:]:
            if (n is None) != (norms[0] is None) or (n is not None and not all(np.array_equal(a, b) for a, b in zip(n, norms[0]))):
                raise ValueError("TD3PopulationTrainer: the critics' action normalisation is shared by all members")
        self._bounds_check(action_bounds, random_timesteps, K, norms)
        self.engine, self.members, self.horizon = engine, members, int(horizon)
        self._templates = []
        for pol, sigma in zip(policies, sigmas):
            t = copy.copy(pol)
            t.log_std = np.full(K + 1, np.log(sigma), np.float32)
            self._templates.append(t)
        self.configs = [dict({k: v for k, v in c.items() if k not in self.SHARED}, critic_widths=hidden + (1,)) for c in cfgs]
        engine.mlp_init(self._templates[0], seeds=agent_seeds, deterministic=False)
        engine.mlp_learners(members)
        for m in range(1, members):
            engine.mlp_set_learner(m, self._templates[m])
        if self.action_bounds is not None:
            engine.mlp_learners_set_bounds(*self.action_bounds)
        engine.rollout_enable(self.horizon, obs=True)
        engine.td3_pop_init(self.configs)
        for m in range(members):
            engine.td3_pop_set_critics(m, critics[m] if critics[m] is not None else random_critics(K, hidden, seeds[m], policies[0].frames), action_norm=norms[0] if m == 0 else None)
        if self.action_bounds is not None:
            engine.td3_pop_set_bounded(True)
        if self.normalize_observations or self.normalize_rewards:
            engine.td3_norm_init(observations=self.normalize_observations, rewards=self.normalize_rewards, per_member=True, **norm)
        self._prio_init(engine, prioritized_replay)
        self._nstep_init(engine, n_step)
        self.history = []

    def set_exploration(self, sigma, member=None):
        """the collection noise's standard deviation of one member (None: of all) from the next day on"""
        for m in range(self.members) if member is None else [int(member)]:
            self._templates[m].log_std = np.full(self._templates[m].num_keywords + 1, np.log(sigma), np.float32)
            self.engine.mlp_set_learner_log_std(m, self._templates[m].log_std)

    def iteration(self, days=None, budget=0.0, reset=False, reset_seeds=None):
        """(reset), `days` (default: the horizon) recorded days of run_days("mlp"), the store, and - once every ring holds
        learning_starts transitions - updates_per_iteration updates; returns the M members' statistics, or only the rings' size
        before that"""
        e = self.engine
        if reset:
            e.reset(seeds=reset_seeds)
        e.rollout_reset()
        if self.action_bounds is not None:
            self._explore_for(e.td3_pop_buffer(fetch=False)["written"])
        e.run_days("mlp", self.horizon if days is None else int(days), budget)
        e.td3_pop_store()
        if self.normalize_observations or self.normalize_rewards:
            e.td3_norm_update()             # (one call for all members, whatever their number)
        size = e.td3_pop_buffer(fetch=False)["size"]
        if size >= self.learning_starts:
            self._prio_anneal()
        stats = e.td3_pop_update(self.updates_per_iteration) if size >= self.learning_starts else dict(buffer_size=size, updates=None)
        self.history.append(stats)
        return stats

    def policy(self, member):
        """an MLPPolicy holding one member's trained actor (its log_std the member's exploration's; under running observation
        normalisers its shift / scale are the member's current vectors)"""
        pol = policy_from_actor(self._templates[member], self.engine.td3_pop_state(member)["theta"])
        return self._squashed(_with_vectors(pol, self.engine.td3_norm_state(member)) if self.normalize_observations else pol)

    def returns(self):
        """[M] float64: per member the mean over its envs of the recorded reward summed over the recorded days"""
        r = self.engine.rollout_fetch()["reward"].astype(np.float64).sum(axis=0)
        return r.reshape(self.members, -1).mean(axis=1)

    def state(self, member, state=None):
        """member's state; `obs_history` (with MLPPolicy(frames > 1)) holds its own envs'"""
        return history_carry(self.engine,
                             lambda w: self._bounded_state(
                                 lambda u: self._nstep_state(lambda t: self._prio_state(lambda s: self.engine.td3_pop_state(member, s), member, t), member, u), w),
                             state, member, self.engine.num_envs // self.members)

    def load_state(self, member, state):
        self.state(member, state)

    def norm_state(self, member, state=None):
        """member's normalisers (TD3Trainer.norm_state's dict; `returns` holds the member's own envs')"""
        return _norm_state(self.engine, member, state, self.engine.num_envs // self.members)


__all__ = ["BoundedActions", "NStepReturns", "PrioritizedReplay", "TD3PopulationTrainer", "TD3Trainer", "td3", "rllib_td3", "random_critics", "actor_params",
           "policy_from_actor"]
