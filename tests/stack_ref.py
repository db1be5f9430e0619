"""The observation history's row law (adcraft_amd/csrc/adc_mlp.h, "Observation history") restated in numpy from the header's
comment.  `History` is the per-env state (hist, last, from); `row` forms the raw stacked row an act on episode day d reads and,
as an act, commits it; a peek writes nothing.  It composes with mlp_ref / pg_ref / td3_ref / sac_ref / norm_ref, which are
general in the row width: feed them the stacked rows."""
import ctypes as C

import numpy as np

F = np.float32
NONE = -2


class History:
    def __init__(self, N, K, frames):
        self.N, self.K, self.H, self.D0 = int(N), int(K), int(frames), 5 * int(K) + 2
        self.hist = np.zeros((self.N, self.H, self.D0), F)
        self.last = np.full(self.N, NONE, np.int32)
        self.frm = np.zeros(self.N, np.int32)

    def copy(self):
        out = History(self.N, self.K, self.H)
        out.hist, out.last, out.frm = self.hist.copy(), self.last.copy(), self.frm.copy()
        return out

    def state(self):
        """StepEngine.mlp_history_state's dict"""
        return {"hist": self.hist.copy(), "last": self.last.copy(), "from": self.frm.copy()}

    def forget(self, mask=None):
        """an explicit reset of the masked envs (None: all)"""
        m = np.ones(self.N, bool) if mask is None else np.asarray(mask, bool)
        self.last[m] = NONE

    def row(self, frame0, day, commit=True):
        """frame0 [N, D0]: the raw flat observation (ignored where day == 0: zeros); day [N]: the envs' episode days.  Returns
        the raw stacked rows [N, H * D0]"""
        frame0, day = np.asarray(frame0, F), np.asarray(day, np.int64)
        out = np.zeros((self.N, self.H * self.D0), F)
        for n in range(self.N):
            d = int(day[n])
            frm = int(self.frm[n])
            if d == 0:
                frm = 0
            elif self.last[n] != d - 1 and self.last[n] != d:
                frm = d
            f0 = np.zeros(self.D0, F) if d == 0 else frame0[n]
            out[n, :self.D0] = f0
            for f in range(1, self.H):
                if d - f >= frm:
                    out[n, f * self.D0:(f + 1) * self.D0] = self.hist[n, (d - f) % self.H]
            if commit:
                self.hist[n, d % self.H] = f0
                self.last[n], self.frm[n] = d, frm
        return out


def twin_row(lib, K, frames, frame0, hist, last, frm, day, commit):
    """adc_mlp_stack_row_host for one env: hist [H, D0] float32, last / frm one-element int32 arrays, all updated in place"""
    D0 = 5 * K + 2
    row = np.zeros(frames * D0, F)
    f0 = None if frame0 is None else np.ascontiguousarray(frame0, F)
    rc = lib.adc_mlp_stack_row_host(K, frames, None if f0 is None else f0.ctypes.data, hist.ctypes.data, last.ctypes.data, frm.ctypes.data,
                                    int(day), 1 if commit else 0, row.ctypes.data)
    assert rc == 0, rc
    return row


def normalized(policy, rows):
    """the network's input from raw stacked rows: per position over the whole row"""
    rows = np.ascontiguousarray(rows, F)
    if policy.shift is None:
        return rows
    with np.errstate(all="ignore"):
        return ((rows - policy.shift[None, :]) * policy.scale[None, :]).astype(F)


def episode_day(out):
    """the envs' episode day after a step's output dict under auto-reset: 0 where the episode ended, else days_passed"""
    done = np.asarray(out["terminated"], bool) | np.asarray(out["truncated"], bool)
    return np.where(done, 0, np.asarray(out["days_passed"]).astype(np.int64))


def random_policy(rng, K, frames, hidden, activation="tanh", two_heads=False, value=False, normalize=False, scale=0.5, **kw):
    """mlp_ref.random_policy on the stacked input: a seeded random MLPPolicy(frames=frames)"""
    from adcraft_amd.baselines.mlp_policy import MLPPolicy
    D, A = frames * (5 * K + 2), K + 1

    def net(widths):
        layers, n_in = [], D
        for n_out in widths:
            layers.append(((rng.standard_normal((n_in, n_out)) * scale / np.sqrt(n_in)).astype(F), (rng.standard_normal(n_out) * 0.1).astype(F)))
            n_in = n_out
        return layers

    if normalize:
        kw["shift"] = (rng.random(D) * 3).astype(F)
        kw["scale"] = (0.01 + rng.random(D) * 0.2).astype(F)
    if not two_heads:
        kw.setdefault("log_std", (rng.standard_normal(A) * 0.5 - 1.0).astype(F))
    return MLPPolicy(net(list(hidden) + [2 * A if two_heads else A]), activation=activation, value_layers=net(list(hidden) + [1]) if value else (),
                     frames=frames, **kw)


# ---- composing with the off-policy restatements --------------------------------------------------------------------------------------
# td3_ref.Shapes (which sac_ref and per_ref use too) takes the row width from the policy's keywords; everything behind it is
# general in the width.  `stacked_shapes()` puts the policy's own input width in its place for the duration of a `with` block,
# so that td3_ref.update / sac_ref.update / per_ref's updates run unedited on stacked rows (frames = 1: the same numbers).
import contextlib

from tests import td3_ref as T3


class Shapes(T3.Shapes):
    def __init__(self, policy, opts):
        super().__init__(policy, opts)
        self.D = policy.input_size
        self.P = sum((i + 1) * o for i, o in zip([self.D] + self.pol_widths[:-1], self.pol_widths))
        self.Qc = sum((i + 1) * o for i, o in zip([self.D + self.A] + self.q_widths[:-1], self.q_widths))


@contextlib.contextmanager
def stacked_shapes():
    old = T3.Shapes
    T3.Shapes = Shapes
    try:
        yield
    finally:
        T3.Shapes = old


def random_critics(rng, K, frames, widths, scale=0.6):
    """td3_ref.random_critics_for_tests on the stacked row: two seeded critics on the frames (5K+2) + K + 1 inputs"""
    out = []
    for _ in range(2):
        layers, n_in = [], frames * (5 * K + 2) + K + 1
        for n_out in widths:
            layers.append(((rng.standard_normal((n_in, n_out)) * scale / np.sqrt(n_in)).astype(F), (rng.standard_normal(n_out) * 0.1).astype(F)))
            n_in = n_out
        out.append(layers)
    return out
