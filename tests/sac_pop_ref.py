"""SAC learner populations against the single-learner law: a member of a population of M learners on N envs owns the envs
[m n, (m + 1) n), n = N / M, its ring takes its own envs' transitions in its own order s = (t - t0) n + local env
(tests/td3_pop_ref.py: MemberRing, slot_order), and everything it computes is what tests/sac_ref.py (the numpy restatement of
csrc/adc_sac.h) computes on that slice of the fetched record under the member's own options and key.  Nothing of the law is
restated here."""
from tests import sac_ref as S
from tests.td3_pop_ref import MemberRing, member_record, member_seed, member_slice, slot_order  # noqa: F401  (the ring order is TD3's)


def member_update(policy, state, buf, opts, engine_seed):
    """adc_engine_sac_pop_update(1) for one member: sac_ref.update on its ring under its key"""
    return S.update(policy, state, buf, member_seed(opts, engine_seed), opts)


def member_fresh_state(policy, critics, opts):
    """a member's state right after sac_pop_init and sac_pop_set_critics(sync_targets=True)"""
    return S.fresh_state(policy, critics, opts)
