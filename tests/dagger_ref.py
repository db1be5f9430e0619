"""numpy restatement of csrc/adc_dagger.h: the per-env coin of a DAgger day.  Word x of the Philox call (0, stage 23, 0, tick)
under the agent's key, against round(beta * 2^32) formed in float32 as adc_law.h's bernoulli_threshold forms it."""
import numpy as np

F = np.float32
ST_DAGGER = 23
TWO32 = F(4294967296.0)


def threshold(beta):
    """round(beta * 2^32) in [0, 2^32]: float32 throughout (the scaling is exact; below 2^23 x + 0.5 is representable)"""
    p = F(beta)
    if not p > F(0):                                    # (NaN too)
        return 0
    x = F(p * TWO32)
    if not x < TWO32:
        return 1 << 32
    return int(x) if x >= F(8388608.0) else int(np.floor(F(x + F(0.5))))


def word(key, tick):
    from oracle import capi as orc
    key = int(key)
    return int(orc.philox([0, ST_DAGGER, 0, int(tick)], [key & 0xFFFFFFFF, key >> 32])[0])


def coin(keys, ticks, beta):
    """uint8 [N]: 1 where the teacher's action is consumed; `ticks` are the agents' ticks BEFORE the day's act"""
    t = threshold(beta)
    return np.array([1 if word(k, c) < t else 0 for k, c in zip(keys, ticks)], dtype=np.uint8)


def mask(keys, tick0, days, beta):
    """uint8 [days, N]: the coins of `days` consecutive DAgger days that start at the agents' ticks tick0 [N]"""
    tick0 = np.asarray(tick0, dtype=np.int64)
    return np.stack([coin(keys, tick0 + d, beta) for d in range(days)])
