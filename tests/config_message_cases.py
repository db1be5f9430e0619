"""The cases behind tests/golden/config_check_messages.json: for every exported adc_*_config_check, adc_*_pop_config_check and
adc_replay_nstep_check a valid configuration, then one case per clause that violates it (NULL, a wrong struct_size, each bound from
either side, a NaN where the clause is written to catch one; for the population checks the members, count and "equal in all
members" clauses).  tools/gen_golden_config_messages.py records what the library answers - (function, case, return code, message) -
and tests/test_config_messages_host.py replays the same list against the library and the g++ host build: code and whole sentence
must be equal.  The case list lives here alone so that the two cannot drift apart."""
import ctypes as C
import json
import math

from adcraft_amd import _ffi

NAN, INF = math.nan, math.inf
i32, MSG = C.c_int32, C.POINTER(C.c_char_p)
K = 3                       # keywords of the MLP cases: A = 4 outputs


def _P(t):
    return C.POINTER(t)


# the checks' signatures (include/adcraft_engine.h), for a library loaded without _ffi.lib()'s table
SIGNATURES = {
    "adc_mlp_config_check": [_P(_ffi.MLPConfig), i32, MSG],
    "adc_es_config_check": [_P(_ffi.ESConfig), MSG],
    "adc_obs_norm_config_check": [_P(_ffi.ObsNormConfig), MSG],
    "adc_rew_norm_config_check": [_P(_ffi.RewNormConfig), MSG],
    "adc_td3_norm_config_check": [_P(_ffi.TD3NormConfig), MSG],
    "adc_sac_norm_config_check": [_P(_ffi.SACNormConfig), MSG],
    "adc_replay_prio_config_check": [_P(_ffi.ReplayPrioConfig), MSG],
    "adc_replay_nstep_check": [i32, MSG],
    "adc_pg_config_check": [_P(_ffi.PGConfig), MSG],
    "adc_pg_pop_config_check": [_P(_ffi.PGConfig), i32, i32, i32, MSG],
    "adc_pg_kl_config_check": [_P(_ffi.PGKLConfig), MSG],
    "adc_pg_shuffle_config_check": [_P(_ffi.PGShuffleConfig), MSG],
    "adc_im_config_check": [_P(_ffi.IMConfig), MSG],
    "adc_td3_config_check": [_P(_ffi.TD3Config), MSG],
    "adc_td3_pop_config_check": [_P(_ffi.TD3Config), i32, i32, i32, MSG],
    "adc_sac_config_check": [_P(_ffi.SACConfig), MSG],
    "adc_sac_pop_config_check": [_P(_ffi.SACConfig), i32, i32, i32, MSG],
    "adc_pbt_config_check": [_P(_ffi.PBTConfig), i32, i32, MSG],
}


def _make(cls, **fields):
    c = cls()
    c.struct_size = C.sizeof(cls)
    for k, v in fields.items():
        if isinstance(v, (tuple, list)):
            for i, x in enumerate(v):
                getattr(c, k)[i] = x
        else:
            setattr(c, k, v)
    return c


def _with(base, **fields):
    """a copy of the configuration `base` with some fields replaced"""
    c = type(base).from_buffer_copy(base)
    for k, v in fields.items():
        if isinstance(v, (tuple, list)):
            for i, x in enumerate(v):
                getattr(c, k)[i] = x
        else:
            setattr(c, k, v)
    return c


def _array(*cfgs):
    return (type(cfgs[0]) * len(cfgs))(*cfgs)


def _three(field, *values):
    """cases (name, {field: value}) named after the field and the value"""
    return [(f"{field}={v!r}", {field: v}) for v in values]


def mlp():
    return _make(_ffi.MLPConfig, activation=_ffi.MLP_TANH, n_policy_layers=2, policy_widths=(8, K + 1, 0, 0), n_value_layers=2, value_widths=(8, 1, 0, 0),
                 normalize=0, clamp_log_std=0, log_std_lo=-1.0, log_std_hi=0.0, bid_clip_hi=0.0, deterministic=0)


def es():
    return _make(_ffi.ESConfig, sigma=0.02, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, l2=0.0, shaping=_ffi.ES_CENTERED_RANK, optimiser=_ffi.ES_ADAM, seed=0)


def pg():
    return _make(_ffi.PGConfig, gamma=0.99, lambda_=0.95, eps_clip=0.2, vf_coef=0.5, ent_coef=0.0, reward_scale=1.0, normalize_advantages=1, max_grad_norm=0.5,
                 optimiser=_ffi.PG_ADAM, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, minibatch_envs=0)


def td3():
    return _make(_ffi.TD3Config, gamma=0.99, tau=0.005, policy_delay=2, target_noise=0.2, target_noise_clip=0.5, action_lo=0.0, action_hi=0.0, reward_scale=1.0,
                 batch_size=16, capacity=64, n_critic_layers=3, critic_widths=(8, 8, 1, 0), actor_lr=1e-3, critic_lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                 optimiser=_ffi.TD3_ADAM, max_grad_norm=0.0, seed=0)


def sac():
    return _make(_ffi.SACConfig, gamma=0.99, tau=0.005, target_update_interval=1, init_alpha=1.0, target_entropy=-4.0, alpha_lr=3e-4, eps_sq=1e-6, reward_scale=1.0,
                 batch_size=16, capacity=64, n_critic_layers=3, critic_widths=(8, 8, 1, 0), actor_lr=1e-3, critic_lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                 optimiser=_ffi.TD3_ADAM, max_grad_norm=0.0, seed=0)


def ring_norm(cls):
    return _make(cls, observations=1, rewards=1, per_member=0, obs_min_std=1e-2, obs_count_cap=0, rew_min_std=1e-2, rew_count_cap=0, rew_clip=10.0)


def pbt(mask=0b1):
    return _make(_ffi.PBTConfig, replace_count=1, fitness_ema=0.0, factor_lo=0.8, factor_hi=1.25, log_factor_lo=-0.2, log_factor_hi=0.2, tuned_mask=mask,
                 lo=(1e-5,) * 8, hi=(1e-2,) * 8, with_ring=0, seed=0)


# the clauses TD3 and SAC share, in the order the checks hold them (the family's own clauses sit between tau and reward_scale)
_OFFPOLICY_HEAD = _three("gamma", -0.1, 1.1, NAN) + _three("tau", 0.0, 1.1, NAN)
_OFFPOLICY_TAIL = (
    _three("reward_scale", 0.0, INF, -INF, NAN) + _three("batch_size", 0, (1 << 20) + 1) + _three("capacity", 0, (1 << 30) + 1) + _three("n_critic_layers", 0, 5) +
    [("last critic width 2", dict(critic_widths=(8, 8, 2, 0))), ("one layer of width 2", dict(n_critic_layers=1, critic_widths=(2, 0, 0, 0)))] +
    _three("actor_lr", -1.0, INF, NAN) + _three("critic_lr", -1.0, INF, NAN) + _three("optimiser", 2, -1) + _three("beta1", -0.1, 1.0, NAN) +
    _three("beta2", -0.1, 1.0, NAN) + _three("eps", 0.0, -1.0, NAN) + _three("max_grad_norm", -1.0, INF, NAN) +
    [("hidden critic width 0", dict(critic_widths=(0, 8, 1, 0))), ("hidden critic width 257", dict(critic_widths=(8, 257, 1, 0))),
     ("SGD ignores Adam's fields", dict(optimiser=_ffi.TD3_SGD, beta1=2.0, beta2=NAN, eps=0.0)), ("one critic layer", dict(n_critic_layers=1, critic_widths=(1, 0, 0, 0))),
     ("a later clause does not hide an earlier one", dict(gamma=2.0, max_grad_norm=-1.0, critic_widths=(0, 8, 1, 0)))])
_TD3_OWN = (_three("policy_delay", 0) + _three("target_noise", -0.1, INF, NAN) + _three("target_noise_clip", -0.1, INF, NAN) + _three("action_lo", NAN) +
            _three("action_hi", NAN) + [("tau before policy_delay", dict(tau=0.0, policy_delay=0)), ("policy_delay before reward_scale", dict(policy_delay=0, reward_scale=0.0))])
_SAC_OWN = (_three("target_update_interval", 0) + _three("init_alpha", 0.0, INF, NAN) + _three("target_entropy", INF, -INF, NAN) + _three("alpha_lr", -1.0, INF, NAN) +
            _three("eps_sq", 0.0, INF, NAN) + [("tau before target_update_interval", dict(tau=0.0, target_update_interval=0)),
                                               ("eps_sq before reward_scale", dict(eps_sq=0.0, reward_scale=0.0))])


def _single(fn, base, variants, extra=()):
    """NULL, a wrong struct_size, the valid configuration, then every variant of it; extra: arguments between cfg and message"""
    yield fn, "NULL", (None, *extra)
    yield fn, "struct_size", (_with(base, struct_size=C.sizeof(type(base)) - 4), *extra)
    yield fn, "valid", (base, *extra)
    for name, fields in variants:
        yield fn, name, (_with(base, **fields), *extra)


def _pop(fn, base, equal_cases, bad_member):
    """the frame the three population checks share: the array, members, count, a member's own check, the equality clauses"""
    two = lambda **f: _array(base, _with(base, **f))                     # noqa: E731
    yield fn, "NULL", (None, 1, 8, 2)
    yield fn, "valid shared", (_array(base), 1, 8, 2)
    yield fn, "valid per member", (_array(base, base), 2, 8, 2)
    yield fn, "num_envs=0", (_array(base), 1, 0, 2)
    yield fn, "members=0", (_array(base), 1, 8, 0)
    yield fn, "members=-1", (_array(base), 1, 8, -1)
    yield fn, "members do not divide num_envs", (_array(base), 1, 8, 3)
    yield fn, "members=65535", (_array(base), 1, 65535 * 2, 65535)
    yield fn, "members=65536", (_array(base), 1, 65536 * 2, 65536)
    yield fn, "count=0", (_array(base), 0, 8, 2)
    yield fn, "count=3 of 2 members", (_array(base, base, base), 3, 8, 2)
    yield fn, "count before the members' own checks", (_array(_with(base, gamma=2.0)), 3, 8, 2)
    yield fn, "first member bad", (_array(_with(base, **bad_member), base), 2, 8, 2)
    yield fn, "second member bad", (two(**bad_member), 2, 8, 2)
    yield fn, "second member struct_size", (two(struct_size=4), 2, 8, 2)
    yield fn, "shared configuration bad", (_array(_with(base, **bad_member)), 1, 8, 2)
    for name, fields in equal_cases:
        yield fn, name, (two(**fields), 2, 8, 2)


def cases():
    """every case as (function, case name, the arguments before `message`)"""
    m = mlp()
    yield from _single("adc_mlp_config_check", m, [
        ("activation=2", dict(activation=2)), ("n_policy_layers=0", dict(n_policy_layers=0)), ("n_policy_layers=5", dict(n_policy_layers=5)),
        ("n_value_layers=-1", dict(n_value_layers=-1)), ("n_value_layers=5", dict(n_value_layers=5)), ("no value network", dict(n_value_layers=0)),
        ("clamp lo > hi", dict(clamp_log_std=1, log_std_lo=1.0, log_std_hi=0.0)), ("clamp lo NaN", dict(clamp_log_std=1, log_std_lo=NAN)),
        ("clamp hi NaN", dict(clamp_log_std=1, log_std_hi=NAN)), ("lo > hi without the clamp", dict(clamp_log_std=0, log_std_lo=1.0, log_std_hi=0.0)),
        ("hidden policy width 0", dict(policy_widths=(0, K + 1, 0, 0))), ("hidden policy width 257", dict(policy_widths=(257, K + 1, 0, 0))),
        ("hidden value width 0", dict(value_widths=(0, 1, 0, 0))), ("hidden value width 257", dict(value_widths=(257, 1, 0, 0))),
        ("policy ends in 5 outputs", dict(policy_widths=(8, 5, 0, 0))), ("two heads", dict(policy_widths=(8, 2 * (K + 1), 0, 0))),
        ("value ends in 2 outputs", dict(value_widths=(8, 2, 0, 0))), ("four layers", dict(n_policy_layers=4, policy_widths=(256, 1, 8, K + 1))),
    ], extra=(K,))
    yield "adc_mlp_config_check", "num_keywords=0", (m, 0)
    yield "adc_mlp_config_check", "num_keywords before activation", (_with(m, activation=2), 0)

    adam = _three("beta1", -0.1, 1.0, NAN) + _three("beta2", -0.1, 1.0, NAN) + _three("eps", 0.0, -1.0, NAN)
    yield from _single("adc_es_config_check", es(), (
        _three("sigma", 0.0, -1.0, INF, NAN) + _three("lr", -1.0, NAN) + _three("shaping", 2) + _three("optimiser", 2) + _three("l2", -1.0, NAN) + adam +
        [("SGD ignores Adam's fields", dict(optimiser=_ffi.ES_SGD, beta1=2.0, beta2=NAN, eps=0.0)), ("lr=inf", dict(lr=INF))]))

    yield from _single("adc_obs_norm_config_check", _make(_ffi.ObsNormConfig, per_member=0, min_std=1e-2, count_cap=0),
                       _three("min_std", 0.0, -1.0, INF, NAN) + _three("count_cap", -1, 1000) + _three("per_member", 1))
    yield from _single("adc_rew_norm_config_check", _make(_ffi.RewNormConfig, per_member=0, min_std=1e-2, clip=10.0, count_cap=0),
                       _three("min_std", 0.0, -1.0, INF, NAN) + _three("clip", -1.0, INF, NAN, 0.0) + _three("count_cap", -1, 1000))
    for fn, cls in (("adc_td3_norm_config_check", _ffi.TD3NormConfig), ("adc_sac_norm_config_check", _ffi.SACNormConfig)):
        yield from _single(fn, ring_norm(cls), (
            [("neither part", dict(observations=0, rewards=0)), ("observations alone", dict(rewards=0)), ("rewards alone", dict(observations=0))] +
            _three("obs_min_std", 0.0, -1.0, INF, NAN) + _three("obs_count_cap", -1) + _three("rew_min_std", 0.0, -1.0, INF, NAN) + _three("rew_count_cap", -1) +
            _three("rew_clip", -1.0, INF, NAN, 0.0) +
            [("the obs clauses hold without observations", dict(observations=0, obs_min_std=0.0)), ("obs before rew", dict(obs_count_cap=-1, rew_min_std=0.0))]))

    yield from _single("adc_replay_prio_config_check", _make(_ffi.ReplayPrioConfig, alpha=0.6, beta=0.4, eps=1e-6, cap=1e6),
                       _three("alpha", -0.1, 1.1, NAN, 0.0, 1.0) + _three("beta", -0.1, 1.1, NAN) + _three("eps", 0.0, INF, NAN) + _three("cap", 1e-6, 0.0, INF, NAN))
    for n in (0, -1, 17, 1, 16):
        yield "adc_replay_nstep_check", f"n={n}", (n,)

    p = pg()
    yield from _single("adc_pg_config_check", p, (
        _three("gamma", -0.1, 1.1, NAN) + _three("lambda_", -0.1, 1.1, NAN) + _three("eps_clip", 1.0, NAN, -1.0) + _three("vf_coef", -1.0, INF, NAN) +
        _three("ent_coef", -1.0, INF, NAN) + _three("reward_scale", 0.0, INF, -INF, NAN) + _three("max_grad_norm", -1.0, INF, NAN) + _three("optimiser", 2) +
        _three("lr", -1.0, INF, NAN) + adam + _three("minibatch_envs", -1, 4) + [("SGD ignores Adam's fields", dict(optimiser=_ffi.PG_SGD, beta1=2.0, beta2=NAN, eps=0.0))]))
    yield from _pop("adc_pg_pop_config_check", p, [
        ("minibatch_envs unequal", dict(minibatch_envs=2)), ("minibatch_envs unequal before a later member's own clause", dict(minibatch_envs=-1)),
    ], dict(gamma=2.0))
    yield "adc_pg_pop_config_check", "minibatch_envs above a member's envs", (_array(_with(p, minibatch_envs=8)), 1, 8, 2)
    yield "adc_pg_pop_config_check", "minibatch_envs does not divide a member's envs", (_array(_with(p, minibatch_envs=3)), 1, 8, 2)
    yield "adc_pg_pop_config_check", "minibatch_envs divides a member's envs", (_array(_with(p, minibatch_envs=2)), 1, 8, 2)

    yield from _single("adc_pg_kl_config_check", _make(_ffi.PGKLConfig, kl_coef=0.2, kl_target=0.01, adaptive=1, factor_up=0.0, factor_down=0.0, vf_clip=0.0), (
        _three("kl_coef", -1.0, INF, NAN) + _three("kl_target", 0.0, INF, NAN) + [("kl_target=0 when not adaptive", dict(adaptive=0, kl_target=0.0))] +
        _three("factor_up", 1.0, INF, NAN, 2.0) + _three("factor_down", 1.0, -0.5, NAN, 0.25) + _three("vf_clip", -1.0, INF, NAN, 0.2)))
    yield from _single("adc_pg_shuffle_config_check", _make(_ffi.PGShuffleConfig, minibatch_samples=64, seed=0, target_kl=0.0),
                       _three("minibatch_samples", 0, -1) + _three("target_kl", -1.0, INF, NAN, 0.02))
    yield from _single("adc_im_config_check", _make(_ffi.IMConfig, beta=0.0, vf_coef=1.0, w_max=20.0, ma_start=100.0, ma_rate=1e-8, train_log_std=1), (
        _three("beta", -1.0, INF, NAN) + _three("vf_coef", -1.0, INF, NAN) + _three("w_max", -1.0, INF, NAN) + _three("ma_start", -1.0, INF, NAN) +
        _three("ma_rate", -0.1, 1.1, NAN)))

    shape = [("n_critic_layers unequal", dict(n_critic_layers=2, critic_widths=(8, 1, 0, 0))), ("critic_widths unequal", dict(critic_widths=(8, 16, 1, 0))),
             ("batch_size unequal", dict(batch_size=32)), ("capacity unequal", dict(capacity=128)), ("batch_size before capacity", dict(batch_size=32, capacity=128)),
             ("the member's own check before the equality clauses", dict(batch_size=0))]
    yield from _single("adc_td3_config_check", td3(), _OFFPOLICY_HEAD + _TD3_OWN + _OFFPOLICY_TAIL)
    yield from _pop("adc_td3_pop_config_check", td3(), shape + [("policy_delay unequal", dict(policy_delay=3)), ("capacity before policy_delay", dict(capacity=128, policy_delay=3)),
                                                                ("policy_delay before the critics' shape", dict(policy_delay=3, critic_widths=(8, 16, 1, 0)))],
                    dict(gamma=2.0))
    yield from _single("adc_sac_config_check", sac(), _OFFPOLICY_HEAD + _SAC_OWN + _OFFPOLICY_TAIL)
    yield from _pop("adc_sac_pop_config_check", sac(), shape + [("target_update_interval unequal", dict(target_update_interval=2)),
                                                                ("capacity before target_update_interval", dict(capacity=128, target_update_interval=2)),
                                                                ("target_update_interval before the critics' shape", dict(target_update_interval=2, critic_widths=(8, 16, 1, 0)))],
                    dict(gamma=2.0))

    PG_, TD3_, SAC_ = _ffi.PBT_PG, _ffi.PBT_TD3, _ffi.PBT_SAC
    b = pbt()
    for kind, kname in ((PG_, "pg"), (TD3_, "td3"), (SAC_, "sac")):
        for fn, name, args in _single("adc_pbt_config_check", b, (
                _three("replace_count", 0, 3) + _three("fitness_ema", -0.1, 1.0, NAN, 0.5) + _three("factor_lo", 0.0, INF, NAN) + _three("factor_hi", 0.0, INF, NAN) +
                _three("log_factor_lo", INF, -INF, NAN) + _three("log_factor_hi", INF, -INF, NAN) + _three("tuned_mask", 1 << 4, 1 << 5, 1 << 6, 0) +
                _three("with_ring", 1, 2, -1) +
                [("lo > hi", dict(lo=(1.0,) + (0.0,) * 7, hi=(0.5,) + (1.0,) * 7)), ("lo=-inf", dict(lo=(-INF,) * 8)), ("hi=inf", dict(hi=(INF,) * 8)),
                 ("lo NaN", dict(lo=(NAN,) * 8)), ("hi NaN", dict(hi=(NAN,) * 8)), ("lo below 0", dict(lo=(-1.0,) * 8)), ("an untuned id is not read", dict(lo=(0.0, NAN) + (0.0,) * 6)),
                 ("id 2: hi=1", dict(tuned_mask=1 << 2, hi=(1.0,) * 8)), ("id 2: hi=0.5", dict(tuned_mask=1 << 2, hi=(0.5,) * 8)),
                 ("id 3: lo=0", dict(tuned_mask=1 << 3, lo=(0.0,) * 8, hi=(0.5,) * 8)), ("id 3: hi=1.5", dict(tuned_mask=1 << 3, hi=(1.5,) * 8)),
                 ("id 3: lo below 0", dict(tuned_mask=1 << 3, lo=(-1.0,) * 8)), ("id 4: lo below 0", dict(tuned_mask=1 << 4, lo=(-1.0,) * 8)),
                 ("id 5: lo below 0", dict(tuned_mask=1 << 5, lo=(-1.0,) * 8)), ("ids 0 and 3: the first bad one", dict(tuned_mask=0b1001, lo=(-1.0,) * 8, hi=(2.0,) * 8))]),
                extra=(4, kind)):
            yield fn, f"{kname}: {name}", args
    yield "adc_pbt_config_check", "kind=2", (b, 4, 2)
    yield "adc_pbt_config_check", "kind=4", (b, 4, 4)
    yield "adc_pbt_config_check", "kind before members", (b, 1, 2)
    yield "adc_pbt_config_check", "members=1", (b, 1, PG_)
    yield "adc_pbt_config_check", "members=0", (b, 0, TD3_)
    yield "adc_pbt_config_check", "members=3: replace_count above members / 2", (_with(b, replace_count=2), 3, SAC_)


def declare(L):
    """give the checks of a ctypes library their signatures"""
    for fn, argtypes in SIGNATURES.items():
        f = getattr(L, fn)
        f.argtypes, f.restype = argtypes, C.c_int
    return L


def run(L):
    """every case against the library L: [function, case, return code, message or None] rows, in cases()'s order"""
    declare(L)
    rows = []
    for fn, name, args in cases():
        msg = C.c_char_p(b"unset")
        rc = getattr(L, fn)(*args, C.byref(msg))
        rows.append([fn, name, int(rc), None if msg.value is None else msg.value.decode()])
    return rows


def dump(rows, path):
    """write run()'s rows as {"cases": {function: [[case, return code, message], ...]}}, one line per function"""
    by_fn = {}
    for fn, name, rc, msg in rows:
        by_fn.setdefault(fn, []).append([name, rc, msg])
    with open(path, "w") as f:
        f.write('{"cases": {\n' + ",\n".join(json.dumps(fn) + ": " + json.dumps(v, separators=(",", ":")) for fn, v in by_fn.items()) + "\n}}\n")


def load(path):
    """the rows dump() wrote, in its order"""
    with open(path) as f:
        return [[fn, name, rc, msg] for fn, v in json.load(f)["cases"].items() for name, rc, msg in v]
