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


__all__ = ["ImitationTrainer", "bc", "marwil"]
