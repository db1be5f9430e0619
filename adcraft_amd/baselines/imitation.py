"""Imitation learning for the device-resident MLP policy: behaviour cloning and MARWIL (Wang et al. 2018, "Exponentially weighted
imitation learning for batched historical data"; RLlib's BC / MARWIL) from the engine's own expert bidders.  A teacher day
(StepEngine.teach_days) has the learner act - its input row and value recorded, its action thrown away - and the teacher act in
its place; `im_update` then descends -(w logp(teacher's action)) + vf_coef * value loss over the record with the
policy-gradient trainer's optimiser, on that trainer's theta.  So the clone is where a PPO / A2C run continues from:
`pg_update` on the learner's own days trains the very parameters imitation left, with a value network fitted to the teacher's
returns.  Everything runs on the device; the arithmetic is csrc/adc_imitation.h; StepEngine.teach_days / im_* are the calls."""
from .mlp_policy import history_carry
from .pg_trainer import policy_from_flat

_IM_KEYS = ("beta", "vf_coef", "w_max", "ma_start", "ma_rate", "train_log_std")
_PG_DEFAULTS = dict(gamma=0.99, max_grad_norm=0.5, optimiser="adam", lr=1e-3)


def bc(**overrides):
    """plain behaviour cloning (RLlib's BC): w = 1, no value loss"""
    cfg = dict(beta=0.0, vf_coef=0.0)
    cfg.update(overrides)
    return cfg


def marwil(**overrides):
    """MARWIL with RLlib's defaults: beta 1, vf_coeff 1, the moving scale from 100 at rate 1e-8"""
    cfg = dict(beta=1.0, vf_coef=1.0, w_max=20.0, ma_start=100.0, ma_rate=1e-8)
    cfg.update(overrides)
    return cfg


class ImitationTrainer:
    """engine: a StepEngine that has been reset (and holds what the teacher needs: agent_init for "zero_margin", interp_init for
    "interpolation", bid curves for "oracle"; for "fixed" the caller writes the action buffers); policy: the MLPPolicy to start
    from; teacher: "oracle", "interpolation", "zero_margin" or "fixed"; horizon: teacher days per iteration; epochs and
    minibatches: how an update is cut (minibatches must divide the engine's envs); beta: 0 clones, > 0 weighs a sample by
    exp(beta adv / c); budget: the teacher's budget override.  Further keywords: StepEngine.im_config's (vf_coef, w_max,
    ma_start, ma_rate, train_log_std) and StepEngine.pg_config's (gamma, reward_scale, lr, max_grad_norm, ...); `vf_coef` among
    them is the imitation loss's.  pg_options: a dict of StepEngine.pg_config's options on top of those - the trainer that later
    fine-tunes with pg_update runs under them, so PPO's own eps_clip, lam, vf_coef, ent_coef go here."""

    def __init__(self, engine, policy, teacher="oracle", horizon=10, epochs=4, beta=0.0, budget=100000.0, minibatches=1, agent_seeds=None,
                 pg_options=None, **options):
        if minibatches < 1 or engine.num_envs % minibatches:
            raise ValueError("minibatches must divide the engine's envs")
        im = {k: options.pop(k) for k in _IM_KEYS if k in options}
        im["beta"] = beta
        self.engine, self._template, self.teacher = engine, policy, teacher
        self.horizon, self.epochs, self.budget = int(horizon), int(epochs), float(budget)
        self.im_config = im
        self.config = dict(dict(_PG_DEFAULTS, **options), **dict(pg_options or {}))
        self.config["minibatch_envs"] = engine.num_envs // int(minibatches)
        engine.mlp_init(policy, seeds=agent_seeds, deterministic=False)
        engine.rollout_enable(self.horizon, obs=True)
        engine.pg_init(**self.config)
        engine.im_init(**im)
        self.history = []

    @classmethod
    def bc(cls, engine, policy, **kw):
        """the behaviour-cloning preset: beta 0, no value loss"""
        return cls(engine, policy, **bc(**kw))

    def iteration(self, reset=False, reset_seeds=None):
        """(reset), `horizon` teacher days, the returns, the update; returns its statistics (and `ma`, the moving scale)"""
        e = self.engine
        if reset:
            e.reset(seeds=reset_seeds)
        e.rollout_reset()
        e.teach_days(self.teacher, self.horizon, self.budget)
        e.im_advantages()
        stats = e.im_update(self.epochs)
        stats["ma"] = e.im_state()["ma"]
        self.history.append(stats)
        return stats

    def policy(self):
        """an MLPPolicy holding the cloned policy layers, value layers and log_std"""
        return policy_from_flat(self._template, self.engine.pg_state()["theta"])

    def state(self, state=None):
        """the trainer's state (StepEngine.pg_state's dict plus `ma` and `calls`; with MLPPolicy(frames > 1) also `obs_history`);
        set: the run continues bit for bit"""
        return history_carry(self.engine, self._state, state)

    def load_state(self, state):
        self.state(state)

    def _state(self, state):
        if state is None:
            st = self.engine.pg_state()
            st.update(self.engine.im_state())
            return st
        self.engine.pg_state(state)
        self.engine.im_state(state)


class DAggerTrainer:
    """DAgger (Ross, Gordon and Bagnell 2011) over StepEngine.dagger_days: in round i the env is driven, env by env, by the teacher
    with probability beta_i = beta0 * beta_decay^i and by the learner otherwise, the teacher labels every visited state, and the
    clone is trained on everything collected so far.  Round 0 at beta0 = 1 is a round of teacher days.

    engine, policy, teacher, epochs, minibatches, budget, agent_seeds, pg_options and the further keywords are ImitationTrainer's
    ("interpolation" cannot teach a DAgger day); rounds x days is the record's horizon.  aggregate=True keeps every round's days in
    the record - `im_advantages` / `im_update` run over all of them, so a round's update costs as many samples as have been
    collected; aggregate=False resets the record before a round and trains on that round alone.  The loss is behaviour cloning:
    MARWIL's weight has no meaning on days the mixture drove, so beta of im_config is 0; the value loss under `vf_coef` fits the
    value network to the mixture's returns.  The record lives on the device and is not part of state()."""

    def __init__(self, engine, policy, teacher="oracle", rounds=10, days=10, epochs=4, beta0=1.0, beta_decay=0.5, aggregate=True,
                 budget=100000.0, minibatches=1, agent_seeds=None, pg_options=None, **options):
        if minibatches < 1 or engine.num_envs % minibatches:
            raise ValueError("minibatches must divide the engine's envs")
        if rounds < 1 or days < 1:
            raise ValueError("rounds and days: at least 1")
        if not 0.0 <= beta0 <= 1.0 or not 0.0 <= beta_decay <= 1.0:
            raise ValueError("beta0 and beta_decay: in [0, 1]")
        if options.pop("beta", 0.0) != 0.0:
            raise ValueError("DAgger clones: the imitation loss's beta is 0 (MARWIL's weight needs returns that follow the labelled action)")
        im = {k: options.pop(k) for k in _IM_KEYS if k in options}
        im["beta"] = 0.0
        self.engine, self._template, self.teacher = engine, policy, teacher
        self.rounds, self.days, self.epochs, self.budget = int(rounds), int(days), int(epochs), float(budget)
        self.beta0, self.beta_decay, self.aggregate = float(beta0), float(beta_decay), bool(aggregate)
        self.im_config = im
        self.config = dict(dict(_PG_DEFAULTS, **options), **dict(pg_options or {}))
        self.config["minibatch_envs"] = engine.num_envs // int(minibatches)
        engine.mlp_init(policy, seeds=agent_seeds, deterministic=False)
        engine.rollout_enable(self.rounds * self.days if self.aggregate else self.days, obs=True)
        engine.pg_init(**self.config)
        engine.im_init(**im)
        self.round, self._recorded = 0, 0
        self.history = []

    def beta(self, round_index=None):
        """the teacher's share of round `round_index` (default: the next one)"""
        return self.beta0 * self.beta_decay ** (self.round if round_index is None else int(round_index))

    def recorded(self):
        """days in the record after the last round"""
        return self._recorded

    def iteration(self, reset=False, reset_seeds=None):
        """(reset), `days` DAgger days at the round's beta, the returns and the update over the record; returns the update's
        statistics with `round`, `beta`, `teacher_share` (of this round's env-days the teacher drove) and `recorded` (days trained on)"""
        e = self.engine
        if self.aggregate and self.round >= self.rounds:
            raise ValueError("the aggregated record is full: the trainer was built for `rounds` rounds")
        if reset:
            e.reset(seeds=reset_seeds)
        if not self.aggregate:
            e.rollout_reset()
        beta = self.beta()
        e.dagger_days(self.teacher, self.days, beta, self.budget)
        mask = e.dagger_mask()
        e.im_advantages()
        stats = e.im_update(self.epochs)
        stats.update(round=self.round, beta=beta, teacher_share=float(mask[-self.days:].mean()), recorded=int(mask.shape[0]),
                     ma=e.im_state()["ma"])
        self.round, self._recorded = self.round + 1, int(mask.shape[0])
        self.history.append(stats)
        return stats

    def policy(self):
        """an MLPPolicy holding the cloned policy layers, value layers and log_std"""
        return policy_from_flat(self._template, self.engine.pg_state()["theta"])

    def state(self, state=None):
        """ImitationTrainer.state's dict plus `round` (the next round's index) and `recorded` (the record's fill level when it was
        taken); set: theta, the optimiser, the moving scale and the round index continue - the record itself stays the engine's"""
        return history_carry(self.engine, self._state, state)

    def load_state(self, state):
        self.state(state)

    def _state(self, state):
        if state is None:
            st = self.engine.pg_state()
            st.update(self.engine.im_state())
            st.update(round=self.round, recorded=self.recorded())
            return st
        self.engine.pg_state(state)
        self.engine.im_state(state)
        self.round = int(state.get("round", self.round))


__all__ = ["ImitationTrainer", "DAggerTrainer", "bc", "marwil"]
