"""A learned bidder for the device: the small fully connected policy (and value) networks the paper trains with PPO / A2C /
TD3 (`fcnet_hiddens [32, 32]` on FlatArrayWrapper observations), held as plain float32 arrays and evaluated by the HIP engine
(StepEngine.mlp_init / mlp_act / mlp_step / run_days("mlp"); the arithmetic is csrc/adc_mlp.h).

The observation is the flat row `buyside_clicks[K] | cost[K] | cumulative_profit | days_passed | impressions[K] | revenue[K] |
sellside_conversions[K]` (D = 5K+2); the action is `[budget, bids...]` (A = K+1).  The policy network ends in A means (with a
free `log_std[A]`) or in 2A values, means then log-stds.

With `frames=H` (1 to 8) the policy acts on the last H observations: its input is H such rows side by side, the newest first
(D = H (5K+2)); the engine gathers the older ones from a per-env history on the device (csrc/adc_mlp.h, observation history).

With `gru=(Wi, bi, Wh, bh)` the policy is recurrent: one GRU cell of width G (torch.nn.GRUCell's arithmetic) stands in front of
the output layer, reads the trunk's last activation (the input row without a trunk) and the env's state, and the output layer
reads the new state (csrc/adc_gru.h).  The state lives on the device, per env; the evolution strategy trains such a policy."""
import ctypes as C

import numpy as np

from .. import _ffi

ACTIVATIONS = {"tanh": _ffi.MLP_TANH, "relu": _ffi.MLP_RELU}
MAX_LAYERS, MAX_WIDTH, MAX_FRAMES = 4, 256, 8
MAX_GRU_WIDTH = 256


def _layers(pairs, what, state_width=0):
    """state_width: the last layer of a recurrent policy reads the cell's state, not the layer before it"""
    pairs, out = list(pairs), []
    for i, (w, b) in enumerate(pairs):
        w = np.ascontiguousarray(w, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
        if w.ndim != 2 or w.shape[1] != b.size:
            raise ValueError(f"{what}: a layer is (W [n_in, n_out], b [n_out])")
        if state_width and i + 1 == len(pairs):
            if w.shape[0] != state_width:
                raise ValueError(f"{what}: the output layer of a recurrent policy reads the cell's state ({state_width} inputs)")
        elif out and out[-1][0].shape[1] != w.shape[0]:
            raise ValueError(f"{what}: layer inputs do not match the previous layer's outputs")
        out.append((w, b))
    return out


def _gru(gru):
    """(Wi [n_in, 3G], bi [3G], Wh [G, 3G], bh [3G]) as float32, input-major, gate order r | z | n"""
    if len(gru) != 4:
        raise ValueError("gru: (Wi [n_in, 3G], bi [3G], Wh [G, 3G], bh [3G])")
    wi, bi, wh, bh = (np.ascontiguousarray(a, dtype=np.float32) for a in gru)
    g = wh.shape[0] if wh.ndim == 2 else 0
    if not 1 <= g <= MAX_GRU_WIDTH:
        raise ValueError(f"gru: the cell's width is 1 to {MAX_GRU_WIDTH}")
    if wi.ndim != 2 or wi.shape[1] != 3 * g or wh.shape != (g, 3 * g) or bi.shape != (3 * g,) or bh.shape != (3 * g,):
        raise ValueError("gru: (Wi [n_in, 3G], bi [3G], Wh [G, 3G], bh [3G])")
    return wi, bi, wh, bh


class MLPPolicy:
    """layers / value_layers: lists of (W [n_in, n_out], b [n_out]) - input-major, i.e. torch's `weight.T`.  log_std [A]: the
    free log standard deviations when the policy ends in A means (default zeros); shift / scale [D]: x' = (x - shift) * scale;
    log_std_clamp (lo, hi); bid_clip: upper clip of the bids in dollars; deterministic: act on the means; frames: the number H
    of observations the input row holds (D = H (5K+2); shift / scale cover all of it)."""

    def __init__(self, layers, activation="tanh", value_layers=(), log_std=None, shift=None, scale=None, log_std_clamp=None,
                 bid_clip=None, deterministic=False, frames=1, gru=None):
        if activation not in ACTIVATIONS:
            raise ValueError(f"unknown activation {activation!r}: 'tanh' or 'relu'")
        self.activation = activation
        if int(frames) != frames or not 1 <= int(frames) <= MAX_FRAMES:
            raise ValueError(f"frames: 1 to {MAX_FRAMES}")
        self.frames = int(frames)
        self.gru = None if gru is None else _gru(gru)
        self.layers = _layers(layers, "policy network", self.gru_width)
        if self.gru is not None:
            if self.frames > 1:
                raise ValueError("a recurrent policy together with the observation history (frames > 1) is not supported")
            n_in = self.layers[-2][0].shape[1] if len(self.layers) > 1 else self.gru[0].shape[0]
            if self.gru[0].shape[0] != n_in:
                raise ValueError(f"gru: Wi reads {self.gru[0].shape[0]} inputs, the cell's input has {n_in}")
        if self.input_size % self.frames or (self.input_size // self.frames) % 5 != 2 or self.input_size // self.frames < 7:
            if self.frames > 1:
                raise ValueError(f"the first layer reads {self.input_size} inputs: not frames = {self.frames} rows of 5K+2")
        self.value_layers = _layers(value_layers, "value network")
        if not 1 <= len(self.layers) <= MAX_LAYERS or len(self.value_layers) > MAX_LAYERS:
            raise ValueError(f"a network has at most {MAX_LAYERS} layers (and the policy network at least one)")
        for net in (self.layers, self.value_layers):
            if any(w.shape[1] > MAX_WIDTH for w, _ in net[:-1]):
                raise ValueError(f"hidden widths are at most {MAX_WIDTH}")
        if self.value_layers and (self.value_layers[-1][0].shape[1] != 1 or self.value_layers[0][0].shape[0] != self.input_size):
            raise ValueError("the value network maps the policy's input to one output")
        if (shift is None) != (scale is None):
            raise ValueError("pass both shift and scale, or neither")
        vec = lambda x, n: None if x is None else np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float32), (n,)))
        self.shift, self.scale = vec(shift, self.input_size), vec(scale, self.input_size)
        self.log_std = None
        if (self.input_size // self.frames) % 5 == 2 and self.output_size == self.num_keywords + 1:
            self.log_std = vec(0.0 if log_std is None else log_std, self.output_size)
        elif log_std is not None:
            raise ValueError("log_std belongs to a policy that ends in K+1 means")
        self.log_std_clamp = None if log_std_clamp is None else (float(log_std_clamp[0]), float(log_std_clamp[1]))
        self.bid_clip = None if bid_clip is None else float(bid_clip)
        self.deterministic = bool(deterministic)

    gru_width = property(lambda self: 0 if self.gru is None else self.gru[2].shape[0])
    input_size = property(lambda self: self.layers[0][0].shape[0] if self.gru is None or len(self.layers) > 1 else self.gru[0].shape[0])
    output_size = property(lambda self: self.layers[-1][0].shape[1])
    num_keywords = property(lambda self: (self.input_size // self.frames - 2) // 5)

    def shapes(self):
        """what StepEngine.mlp_init fixes and mlp_set_weights must find again: every layer's shape, the head's free log_std,
        whether there is a normalisation"""
        return ([w.shape for w, _ in self.layers], [w.shape for w, _ in self.value_layers], self.log_std is not None,
                self.shift is not None) + ((self.frames,) if self.frames > 1 else ()) + ((("gru",) + tuple(a.shape for a in self.gru),) if self.gru else ())

    @classmethod
    def from_arrays(cls, layers, **kw):
        return cls(layers, **kw)

    @classmethod
    def from_torch(cls, module, value_module=None, cell=None, head=None, **kw):
        """a torch.nn.Sequential that is exactly Linear, act, Linear, act, ..., Linear with act = Tanh or ReLU (one kind for
        the policy and the value network): what the engine evaluates.  Any other structure - an activation after the last
        Linear, two Linear in a row, a leading activation - is refused, not converted into a different function.

        Recurrent: from_torch(trunk, cell=torch.nn.GRUCell, head=torch.nn.Linear).  `trunk` is None (the cell reads the input row)
        or a Sequential Linear, act, ..., Linear, act - every trunk layer is followed by its activation; torch's [3G, n_in] gate
        blocks (r | z | n rows) become the input-major [n_in, 3G] the engine holds."""
        import torch
        if (cell is None) != (head is None):
            raise ValueError("a recurrent policy is from_torch(trunk, cell=GRUCell, head=Linear): pass both cell and head")
        if cell is not None:
            if not isinstance(cell, torch.nn.GRUCell) or not isinstance(head, torch.nn.Linear):
                raise ValueError(f"unsupported module {type(cell).__name__} / {type(head).__name__}: cell is a GRUCell, head a Linear")
            if not cell.bias:
                raise ValueError("the GRUCell must have biases (bias=True)")
            t = lambda p: p.detach().cpu().numpy()
            kw["gru"] = (t(cell.weight_ih).T.copy(), t(cell.bias_ih).copy(), t(cell.weight_hh).T.copy(), t(cell.bias_hh).copy())
            trunk = [] if module is None else list(module)
            if trunk and not isinstance(trunk[-1], (torch.nn.Tanh, torch.nn.ReLU)):
                raise ValueError("policy network: a recurrent policy's trunk ends with the activation of its last Linear")
            module = torch.nn.Sequential(*trunk, head)

        def unpack(seq, what):
            mods = list(seq)
            if len(mods) % 2 == 0 or not all(isinstance(m, torch.nn.Linear) for m in mods[0::2]):
                for m in mods:
                    if not isinstance(m, (torch.nn.Linear, torch.nn.Tanh, torch.nn.ReLU)):
                        raise ValueError(f"unsupported module {type(m).__name__}: Linear, Tanh and ReLU only")
                raise ValueError(f"{what}: the modules must alternate Linear, activation, ..., and begin and end with a Linear")
            pairs, acts = [], set()
            for m in mods[0::2]:
                bias = m.bias.detach() if m.bias is not None else torch.zeros(m.out_features)
                pairs.append((m.weight.detach().cpu().numpy().T.copy(), bias.cpu().numpy().copy()))
            for m in mods[1::2]:
                if isinstance(m, torch.nn.Tanh):
                    acts.add("tanh")
                elif isinstance(m, torch.nn.ReLU):
                    acts.add("relu")
                elif isinstance(m, torch.nn.Linear):
                    raise ValueError(f"{what}: two Linear modules in a row (an activation goes between them)")
                else:
                    raise ValueError(f"unsupported module {type(m).__name__}: Linear, Tanh and ReLU only")
            return pairs, acts

        pairs, acts = unpack(module, "policy network")
        vpairs, vacts = unpack(value_module, "value network") if value_module is not None else ([], set())
        acts |= vacts
        if len(acts) > 1:
            raise ValueError("one kind of activation per policy")
        if acts and kw.setdefault("activation", next(iter(acts))) not in acts:
            raise ValueError(f"activation={kw['activation']!r} is not what the modules hold")
        return cls(pairs, value_layers=vpairs, **kw)

    def config(self, num_keywords, deterministic=None):
        """the engine's adc_mlp_config for an engine of num_keywords keywords (ValueError when the shapes do not fit)"""
        c = _ffi.MLPConfig()
        c.struct_size = C.sizeof(_ffi.MLPConfig)
        c.activation = ACTIVATIONS[self.activation]
        c.n_policy_layers, c.n_value_layers = len(self.layers), len(self.value_layers)
        for i, (w, _) in enumerate(self.layers):
            c.policy_widths[i] = w.shape[1]
        for i, (w, _) in enumerate(self.value_layers):
            c.value_widths[i] = w.shape[1]
        c.normalize = 0 if self.shift is None else 1
        c.clamp_log_std = 0 if self.log_std_clamp is None else 1
        c.log_std_lo, c.log_std_hi = self.log_std_clamp or (0.0, 0.0)
        c.bid_clip_hi = self.bid_clip or 0.0
        c.deterministic = 1 if (self.deterministic if deterministic is None else deterministic) else 0
        if self.gru is not None and self.layers[-1][0].shape[1] not in (int(num_keywords) + 1, 2 * (int(num_keywords) + 1)):
            raise ValueError("the policy network ends in num_keywords + 1 outputs (means) or twice that (means, log-stds)")
        if self.input_size != self.frames * (5 * int(num_keywords) + 2):
            raise ValueError(f"the policy reads {self.input_size} inputs, the engine's observation has {5 * int(num_keywords) + 2}"
                             + (f" (times frames = {self.frames})" if self.frames > 1 else ""))
        msg = C.c_char_p()
        if _ffi.lib().adc_mlp_config_check(C.byref(c), int(num_keywords), C.byref(msg)) != _ffi.ADC_OK:
            raise ValueError((msg.value or b"bad MLP configuration").decode())
        return c


def history_carry(engine, get_or_set, state, member=0, envs=None):
    """get_or_set(state): a trainer's own state call; the policy's observation history rides along as `obs_history` (all envs',
    or the `envs` of a member), so that a resumed run continues bit for bit.  Nothing is added without one (frames = 1)."""
    sl = slice(None) if envs is None else slice(member * envs, (member + 1) * envs)
    if state is None:
        st = get_or_set(None)
        hist = engine.mlp_history_state()
        if hist is not None:
            st["obs_history"] = {k: v[sl].copy() for k, v in hist.items()}
        return st
    state = dict(state)
    hist = state.pop("obs_history", None)
    out = get_or_set(state)
    if hist is not None:
        now = engine.mlp_history_state()
        if now is None:
            raise ValueError("the state carries an observation history and the policy has none (frames = 1)")
        for k in now:
            now[k][sl] = hist[k]
        engine.mlp_set_history_state(now)
    return out


__all__ = ["MLPPolicy", "history_carry"]
