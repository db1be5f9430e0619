"""TD3 learner populations against the single-learner law: a member of a population of M learners on N envs owns the envs
[m n, (m + 1) n), n = N / M, its ring takes its own envs' transitions in its own order s = (t - t0) n + local env, and
everything it computes is what tests/td3_ref.py (the numpy restatement of csrc/adc_td3.h) computes on that slice of the fetched
record under the member's own options and key.  Nothing of the law is restated here except the member's ring order, which is
written out once more (slot_order) so that it can be held against td3_ref.Ring on the slice."""
import numpy as np

from tests import td3_ref as T3

F = np.float32


def member_slice(m, n):
    return slice(m * n, (m + 1) * n)


def member_record(rec, m, n):
    """the member's columns of rollout_fetch's dict ([T, N, ...] arrays; bootstrap_value [N])"""
    sl = member_slice(m, n)
    return {k: (np.ascontiguousarray(v[sl]) if k == "bootstrap_value" else np.ascontiguousarray(v[:, sl])) for k, v in rec.items()}


def member_seed(opts, engine_seed):
    """the seed of the member's td3 key: its configuration's, or the engine's when that is 0"""
    return opts["seed"] or engine_seed


def slot_order(N, M, m, T, C, written=0, t0=0):
    """the population's store of the recorded days [t0, T) for member m: a list of (slot, t, env) in the order written, env the
    engine's env index; samples a later sample of the same store overwrites are left out (the skip rule)"""
    n = N // M
    count = (T - t0) * n
    out = []
    for s in range(count):
        if s + C < count:
            continue
        out.append(((written + s) % C, t0 + s // n, m * n + s % n))
    return out


class MemberRing(T3.Ring):
    """member m's ring of a population on N envs: td3_ref.Ring fed with the member's slice of the record"""

    def __init__(self, capacity, D, A, m, n):
        super().__init__(capacity, D, A)
        self.m, self.n = m, n

    def store(self, rec, current_input, t0=0):
        """rec: the whole engine's rollout_fetch dict; current_input [N, D]"""
        super().store(member_record(rec, self.m, self.n), current_input[member_slice(self.m, self.n)], t0)


def member_update(policy, state, buf, norm, opts, engine_seed):
    """adc_engine_td3_pop_update(1) for one member: td3_ref.update on its ring under its key"""
    return T3.update(policy, state, buf, norm, member_seed(opts, engine_seed), opts)
