"""Learner populations against the single-learner law: a member of a population of M learners on N envs owns the envs
[m n, (m + 1) n), n = N / M, and everything it computes is what tests/pg_ref.py (the numpy restatement of csrc/adc_pg.h)
computes on that slice of the fetched record under the member's own options.  Nothing of the law is restated here: these
helpers cut the slice and call pg_ref as it is."""
import numpy as np

from tests import pg_ref as P

F = np.float32


def member_slice(m, n):
    return slice(m * n, (m + 1) * n)


def member_record(rec, m, n):
    """the member's columns of rollout_fetch's dict ([T, N, ...] arrays; bootstrap_value [N])"""
    sl = member_slice(m, n)
    return {k: (np.ascontiguousarray(v[sl]) if k == "bootstrap_value" else np.ascontiguousarray(v[:, sl])) for k, v in rec.items()}


def member_gae(rec, m, n, opts):
    """(adv, ret) [T, n] of the member: GAE and - if its options ask for it - the normalisation over its own T n samples"""
    r = member_record(rec, m, n)
    return P.gae(r["reward"], r["terminated"], r["truncated"], r["value"], r["bootstrap_value"], **opts)


def member_update(policy, state, rec, m, n, epochs, opts):
    """adc_engine_pg_pop_update for member m: pg_ref.update on its slice (opts["minibatch_envs"] counts the member's envs)"""
    r = member_record(rec, m, n)
    return P.update(policy, state, r, r["bootstrap_value"], epochs, opts)


def member_minibatch(policy, state, rec, adv, ret, m, n, index, opts):
    """adc_engine_pg_pop_minibatch(index) for member m; adv / ret [T, N] as fetched"""
    r = member_record(rec, m, n)
    mb = opts["minibatch_envs"] or n
    sl = member_slice(m, n)
    return P.minibatch(policy, state, r, np.ascontiguousarray(adv[:, sl]), np.ascontiguousarray(ret[:, sl]), index * mb, mb, opts)


def fresh_state(policy):
    theta = P.flat_params(policy)
    return dict(theta=theta, m=np.zeros_like(theta), v=np.zeros_like(theta), steps=0)
