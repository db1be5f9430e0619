"""The MLP policy on the host: adc_mlp_act_host (the code the device kernel runs, adc_mlp.h) against the numpy restatement in
tests/mlp_ref.py bit for bit, against torch's float32 forward by the yardstick of a float64 forward, the law's own tanh / exp
over every float32 in [-20, 20], and the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

from tests import mlp_ref as R

F = np.float32


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _assert_act(twin, ref, row, what):
    for k in ("mean", "log_std", "action", "logp", "value", "bids", "budget"):
        assert _same(twin[k][0], ref[k][row]), (what, k, twin[k][0], ref[k][row])


def _rows(rng, K, B):
    obs = R.realistic_obs(rng, B, K)
    obs[0] = 0.0                                   # a first day
    obs[1, :K] = rng.integers(10 ** 6, 2 ** 30, K).astype(F)       # large counts
    obs[1, 2 * K] = F(-9.9e6)
    return obs


@pytest.mark.parametrize("K", [1, 7, 100, 256])
@pytest.mark.parametrize("hidden", [(32, 32), (64,), (256, 128, 64)])
def test_twin_equals_the_restatement_bit_for_bit(lib, K, hidden):
    """means, log-stds, actions, log-probability, value, cent bids and budget over seeded random networks: tanh and relu, both
    head layouts, with and without normalisation and value network, stochastic / deterministic / replayed normals"""
    rng = np.random.default_rng(1000 * K + len(hidden))
    A, B = K + 1, 4
    case = 0
    for activation in ("tanh", "relu"):
        for two_heads in (False, True):
            normalize, value = case in (1, 2), case in (0, 1)           # (each head layout with and without either)
            clamp = (-3.0, 0.5) if case % 3 == 0 else None
            clip = 3.0 if case % 3 == 1 else None
            pol = R.random_policy(rng, K, hidden, activation, two_heads, value, normalize, scale=1.5 if normalize else 0.02,
                                  log_std_clamp=clamp, bid_clip=clip)
            obs = _rows(rng, K, B)
            # replayed normals
            z = rng.standard_normal((B, A)).astype(F)
            ref = R.act(pol, obs, z)
            for r in range(B):
                _assert_act(R.twin_act(lib, pol, None if r == 0 else obs[r], z[r]), ref, r, (case, "replay", r))
            # the agent's own stream
            seeds = rng.integers(0, 2 ** 63, B)
            keys = [R.agent_key(s) for s in seeds]
            assert [lib.adc_mlp_agent_key_host(int(s)) for s in seeds] == keys
            assert lib.adc_mlp_default_agent_key_host(int(seeds[0]), 4096 + case) == R.default_agent_key(seeds[0], 4096 + case)
            ticks = rng.integers(0, 1000, B)
            zs = R.normals(keys, ticks, A)
            assert np.all(np.isfinite(zs)) and (A < 64 or 0.5 < zs.std() < 1.5)
            ref = R.act(pol, obs, zs, budget_override=123.5)
            for r in range(B):
                _assert_act(R.twin_act(lib, pol, obs[r], None, keys[r], ticks[r], budget_override=123.5), ref, r, (case, "own", r))
            # deterministic
            ref = R.act(pol, obs, None, deterministic=True)
            for r in range(B):
                t = R.twin_act(lib, pol, obs[r], None, deterministic=True)
                _assert_act(t, ref, r, (case, "det", r))
                assert _same(t["action"], t["mean"])
            case += 1


def test_twin_with_a_nan_and_an_infinity_in_the_means(lib):
    """a NaN mean bids one cent, an infinite one the ceiling (or the clip); both restated bit for bit"""
    rng = np.random.default_rng(5)
    K = 7
    for clip in (None, 2.5):
        pol = R.random_policy(rng, K, (32, 32), "relu", bid_clip=clip)
        w, b = pol.layers[-1]
        b[2], b[3], b[4], b[0] = np.nan, np.inf, -np.inf, np.nan
        obs = _rows(rng, K, 3)
        z = rng.standard_normal((3, K + 1)).astype(F)
        ref = R.act(pol, obs, z)
        for r in range(3):
            t = R.twin_act(lib, pol, obs[r], z[r])
            _assert_act(t, ref, r, (clip, r))
            assert t["bids"][0, 1] == F(0.01) and t["bids"][0, 3] == F(0.01) and t["budget"][0] == F(0.01)
            assert t["bids"][0, 2] == (F(clip) if clip else F(1.0e7))


def _torch_policy(torch, K, hidden, act, seed):
    torch.manual_seed(seed)
    mods, n_in = [], 5 * K + 2
    for h in hidden:
        mods += [torch.nn.Linear(n_in, h), torch.nn.Tanh() if act == "tanh" else torch.nn.ReLU()]
        n_in = h
    mods.append(torch.nn.Linear(n_in, K + 1))
    net = torch.nn.Sequential(*mods)
    with torch.no_grad():                       # means spread over about $0 - $2
        net[-1].weight.mul_(3.0)
        net[-1].bias.add_(1.0)
    return net


@pytest.mark.parametrize("K", [10, 100, 256])
def test_twin_is_as_close_to_float64_as_torch_and_agrees_on_cents(lib, K):
    """from_torch policies on rows of realistic magnitude: the twin's means against a float64 forward of the same network are
    allowed 4 x torch's own float32 maximum error on the same rows; cent bids differ from torch's in at most 1 of 1000"""
    import torch
    from adcraft_amd.baselines.mlp_policy import MLPPolicy
    rng = np.random.default_rng(77 + K)
    B = 64
    shift, scale = R.realistic_norm(K)
    obs = R.realistic_obs(rng, B, K)
    x32 = ((obs - shift) * scale).astype(F)
    lines = []
    for act in ("tanh", "relu"):
        net = _torch_policy(torch, K, (32, 32), act, K)
        pol = MLPPolicy.from_torch(net, shift=shift, scale=scale, deterministic=True)
        assert pol.activation == act and len(pol.layers) == 3
        with torch.no_grad():
            y32 = net(torch.from_numpy(x32)).numpy()
            y64 = net.double()(torch.from_numpy(x32.astype(np.float64))).numpy()
        twin = np.stack([R.twin_act(lib, pol, obs[r])["mean"][0] for r in range(B)])
        err_torch = float(np.abs(y32.astype(np.float64) - y64).max())
        err_twin = float(np.abs(twin.astype(np.float64) - y64).max())
        cents_twin, cents_torch = R.cent_bids(twin[:, 1:]), R.cent_bids(y32[:, 1:])
        share = float(np.mean(cents_twin != cents_torch))
        lines.append(f"K={K} [32,32] {act}: max |mean - float64 forward| twin {err_twin:.3e}, torch float32 {err_torch:.3e} "
                     f"(ratio {err_twin / err_torch:.2f}); cent bids differing from torch's {share:.2e} of {cents_twin.size}")
        print(lines[-1])
        assert 0.2 < float(y64[:, 1:].mean()) < 2.5
        assert err_twin <= 4.0 * err_torch, lines[-1]
        assert share <= 1.0e-3, lines[-1]


def test_from_torch_refuses_what_the_engine_would_not_reproduce():
    """only Linear, act, Linear, ..., Linear is converted: an activation after the last Linear (a squashed head), two Linear in a
    row, a leading activation, an empty module or mixed activations would be evaluated as another function, so they are refused"""
    import torch
    from adcraft_amd.baselines.mlp_policy import MLPPolicy
    nn, K = torch.nn, 3
    D, A = 5 * K + 2, K + 1
    good = nn.Sequential(nn.Linear(D, 8), nn.Tanh(), nn.Linear(8, A))
    value = nn.Sequential(nn.Linear(D, 8), nn.Tanh(), nn.Linear(8, 1))
    bad = [nn.Sequential(nn.Linear(D, 8), nn.Tanh(), nn.Linear(8, A), nn.Tanh()),
           nn.Sequential(nn.Linear(D, 8), nn.Linear(8, A), nn.Tanh()),
           nn.Sequential(nn.Tanh(), nn.Linear(D, 8), nn.Linear(8, A)),
           nn.Sequential(nn.Linear(D, 8), nn.Linear(8, 8), nn.Linear(8, A)),
           nn.Sequential(nn.Linear(D, 8), nn.Tanh(), nn.ReLU(), nn.Linear(8, A)),
           nn.Sequential()]
    for net in bad:
        with pytest.raises(ValueError, match="Linear"):
            MLPPolicy.from_torch(net)
        with pytest.raises(ValueError, match="Linear"):
            MLPPolicy.from_torch(good, value_module=nn.Sequential(*list(net)[:-1], nn.Linear(8, 1), nn.Tanh()) if len(net) else net)
    with pytest.raises(ValueError, match="one kind"):
        MLPPolicy.from_torch(nn.Sequential(nn.Linear(D, 8), nn.Tanh(), nn.Linear(8, 8), nn.ReLU(), nn.Linear(8, A)))
    with pytest.raises(ValueError, match="one kind"):
        MLPPolicy.from_torch(good, value_module=nn.Sequential(nn.Linear(D, 8), nn.ReLU(), nn.Linear(8, 1)))
    with pytest.raises(ValueError, match="activation"):
        MLPPolicy.from_torch(good, activation="relu")
    pol = MLPPolicy.from_torch(good, value_module=value)
    assert pol.activation == "tanh" and len(pol.layers) == 2 and len(pol.value_layers) == 1 + 1
    assert MLPPolicy.from_torch(nn.Sequential(nn.Linear(D, A))).activation == "tanh"          # a single Linear: nothing to choose
    assert np.array_equal(pol.layers[0][0], good[0].weight.detach().numpy().T)


def test_own_tanh_and_exp_over_every_float32_in_range(lib):
    """every float32 in [-20, 20]: tanh is odd, monotone and bounded by 1, exp monotone; the errors against float64 libm are printed"""
    out, bad = (C.c_double * 3)(), (C.c_int64 * 4)()
    n = lib.adc_mlp_math_sweep_host(0, -20.0, 20.0, out, bad)
    print(f"tanh: {n} values, max abs error {out[0]:.3e}, max ulp error {out[1]:.4f}, max |tanh| {out[2]}")
    assert n == 2 * 0x41A00000 + 1
    assert list(bad) == [0, 0, 0, 0] and out[2] <= 1.0
    n = lib.adc_mlp_math_sweep_host(1, -20.0, 20.0, out, bad)
    print(f"exp: {n} values, max abs error {out[0]:.3e}, max ulp error {out[1]:.4f}")
    assert list(bad) == [0, 0, 0, 0]
    x = np.concatenate([np.linspace(-20, 20, 4001), [0.0, -0.0, 1e-30, 0.17, 0.1699, 9.99, 10.0, 88.0, 90.0, -87.0, -100.0]]).astype(F)
    assert _same(np.array([lib.adc_mlp_math_host(0, float(v)) for v in x], F), R.tanh32(x))
    assert _same(np.array([lib.adc_mlp_math_host(1, float(v)) for v in x], F), R.exp32(x))
    assert np.isnan(lib.adc_mlp_math_host(0, float("nan"))) and np.isnan(lib.adc_mlp_math_host(1, float("nan")))


def test_refusals_without_a_device(lib):
    """unknown activation, width > 256, more than 4 layers, a head that is neither A nor 2A, a foreign module; a sharded engine
    refuses the calls by name"""
    from adcraft_amd import _ffi
    from adcraft_amd.baselines.mlp_policy import MLPPolicy
    from adcraft_amd.engine import ShardedStepEngine, StepEngine
    K = 3
    D, A = 5 * K + 2, K + 1
    z = lambda i, o: (np.zeros((i, o), F), np.zeros(o, F))
    with pytest.raises(ValueError, match="activation"):
        MLPPolicy([z(D, A)], activation="gelu")
    with pytest.raises(ValueError, match="256"):
        MLPPolicy([z(D, 257), z(257, A)])
    with pytest.raises(ValueError, match="4 layers"):
        MLPPolicy([z(D, 8), z(8, 8), z(8, 8), z(8, 8), z(8, A)])
    with pytest.raises(ValueError, match="outputs"):
        MLPPolicy([z(D, 8), z(8, A + 1)]).config(K)
    with pytest.raises(ValueError, match="inputs"):
        MLPPolicy([z(D, A)]).config(K + 1)
    with pytest.raises(ValueError, match="one output"):
        MLPPolicy([z(D, A)], value_layers=[z(D, 2)])
    assert MLPPolicy([z(D, 2 * A)]).config(K).n_policy_layers == 1
    # the C side makes the same checks on a raw configuration
    ok = MLPPolicy([z(D, 8), z(8, A)]).config(K)
    msg = C.c_char_p()

    def refused(**kw):
        c = _ffi.MLPConfig.from_buffer_copy(ok)
        for k, v in kw.items():
            if isinstance(v, list):
                for i, x in enumerate(v):
                    getattr(c, k)[i] = x
            else:
                setattr(c, k, v)
        return lib.adc_mlp_config_check(C.byref(c), K, C.byref(msg)) == _ffi.ADC_EINVAL

    assert lib.adc_mlp_config_check(C.byref(ok), K, C.byref(msg)) == _ffi.ADC_OK
    assert refused(activation=2) and b"activation" in msg.value
    assert refused(policy_widths=[257, A, 0, 0]) and b"256" in msg.value
    assert refused(n_policy_layers=5) and b"4 layers" in msg.value
    assert refused(policy_widths=[8, A + 2, 0, 0]) and b"outputs" in msg.value
    assert refused(n_value_layers=1, value_widths=[3, 0, 0, 0])
    assert refused(struct_size=4)
    import torch
    with pytest.raises(ValueError, match="unsupported module"):
        MLPPolicy.from_torch(torch.nn.Sequential(torch.nn.Linear(D, 8), torch.nn.Sigmoid(), torch.nn.Linear(8, A)))
    assert StepEngine.POLICIES["mlp"] == 4
    sharded = object.__new__(ShardedStepEngine)
    for name in ("mlp_init", "mlp_set_weights", "mlp_act", "mlp_step", "mlp_last", "rollout_enable", "rollout_reset", "rollout_fetch"):
        with pytest.raises(NotImplementedError, match="engine_shards=1"):
            getattr(sharded, name)
