"""The SAC kind of the population-based training scheduler's law (adcraft_amd/csrc/adc_pbt.h: "explore", "alpha", "then")
restated in numpy from the header's comments, on top of tests/pbt_ref.py (fitness, smoothing, ranking, donor draw, the product
explore and its clamp) and tests/sac_ref.py (the law's exp).  adc_pbt_explore_host(kind 3), k_pbt_exploit_cell and
adc_engine_pbt_step over a SAC population must give these very bits."""
import numpy as np

from tests import pbt_ref as B
from tests import sac_ref as S

F = np.float32
SAC = 3
SAC_IDS = ("actor_lr", "critic_lr", "alpha_lr", "tau", "alpha", "target_entropy")
ALPHA = 4
HOST_IDS = tuple(h for h in range(len(SAC_IDS)) if h != ALPHA)       # what lives in the member's adc_sac_config


def explore(cfg, bits, donor, own):
    """[8] float32: the replaced member's values by id; ids 0-3 and 5 are the donor's times a factor, clamped (a negative
    target_entropy takes the same product and compares); id 4 is the device's cell and stays what `own` says"""
    host = dict(cfg, tuned_mask=int(cfg["tuned_mask"]) & ~(1 << ALPHA))
    return B.explore(host, B.PG, bits, donor, own)


def shift_of(cfg, bits):
    """the log-domain shift a replaced member's log_alpha gets before the clamp; 0 with alpha untuned"""
    if not (int(cfg["tuned_mask"]) >> ALPHA) & 1:
        return F(0)
    return F(cfg["log_factor_hi"] if (int(bits) >> ALPHA) & 1 else cfg["log_factor_lo"])


def cell_after(cfg, bits, donor_la3):
    """(log_alpha3 [3], alpha) of a replaced member from its donor's {log_alpha, m, v}: untuned, the donor's verbatim; tuned,
    la' = clamp(la + shift) (one float32 sum), m and v the donor's; alpha = the law's exp of la'"""
    la3 = np.array(donor_la3, dtype=F)
    if (int(cfg["tuned_mask"]) >> ALPHA) & 1:
        with np.errstate(all="ignore"):
            la3[0] = B.clamp(F(la3[0] + shift_of(cfg, bits)), cfg["lo"][ALPHA], cfg["hi"][ALPHA])
    return la3, S.alpha_of(la3[0])


def hp_of(opts):
    """[M, 8] float32 from the members' option dicts; id 4 is 0: the temperature is not in the configuration"""
    hp = np.zeros((len(opts), 8), F)
    for m, o in enumerate(opts):
        for h in HOST_IDS:
            hp[m, h] = o[SAC_IDS[h]]
    return hp


def round_(cfg, seed, state, fit, hp):
    """one round on (state = dict(round, smoothed [M]), fit [M], hp [M, 8] as hp_of's).  Returns (new state, result dict as
    StepEngine.pbt_step's plus bits; hp's id 4: the log shift of a replaced member, 0 else)"""
    M = len(fit)
    s = B.smooth(cfg["fitness_ema"], state["smoothed"], fit, state["round"] == 0)
    rank, src, bits = B.plan(seed, state["round"], cfg["replace_count"], s)
    hp_new = np.array(hp, dtype=F)
    hp_new[:, ALPHA] = 0
    s_new = s.copy()
    for m in range(M):
        if src[m] < 0:
            continue
        hp_new[m] = explore(cfg, bits[m], hp[src[m]], hp[m])
        hp_new[m, ALPHA] = shift_of(cfg, bits[m])
        s_new[m] = s[src[m]]
    return (dict(round=state["round"] + 1, smoothed=s_new),
            dict(fitness=np.asarray(fit, np.float64).copy(), smoothed=s_new, rank=rank, src=src, hp=hp_new, bits=bits))
