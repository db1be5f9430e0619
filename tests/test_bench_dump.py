"""bench.py --dump-outputs without a GPU: what dump_outputs writes from the arrays a step returns (float32 / float64 files, the
64 MB cap by a fixed sample of env rows, the same files every time)."""
import os

import numpy as np

import bench


def _step_like(N, K, seed=0):
    """arrays with the dtypes and shapes of StepEngine.fetch()"""
    rng = np.random.default_rng(seed)
    nk = lambda dt: rng.integers(0, 300, (N, K)).astype(dt)        # noqa: E731
    return {"impressions": nk(np.int32), "buyside_clicks": nk(np.int32), "sellside_conversions": nk(np.int32),
            "cost": rng.random((N, K), np.float32), "revenue": rng.random((N, K), np.float32),
            "reward": rng.random(N), "cumulative_profit": rng.random(N), "days_passed": rng.integers(0, 60, N).astype(np.int32),
            "terminated": rng.integers(0, 2, N).astype(np.uint8), "truncated": rng.integers(0, 2, N).astype(np.uint8)}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_every_output_exactly_as_float32_or_float64(tmp_path):
    out = _step_like(8, 16)
    bench.dump_outputs(out, str(tmp_path / "d"))
    got = _load(tmp_path / "d")
    assert set(got) == set(out) | {"env_index"}
    for k, v in out.items():
        assert got[k].dtype == (np.float64 if v.dtype == np.float64 else np.float32), k
        assert got[k].shape == v.shape and np.array_equal(got[k], v), k
    assert got["env_index"].dtype == np.float64 and np.array_equal(got["env_index"], np.arange(8))


def test_dump_over_the_limit_keeps_the_same_seeded_rows_of_every_output(tmp_path):
    N, K = 300, 64
    out = _step_like(N, K, seed=1)
    limit = 200 << 10
    for d in ("a", "b"):
        bench.dump_outputs(out, str(tmp_path / d), limit_bytes=limit)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= limit
    rows = a["env_index"].astype(np.int64)
    assert 0 < len(rows) < N and (np.diff(rows) > 0).all() and rows[-1] < N
    for k, v in out.items():
        assert np.array_equal(a[k], v[rows]), k
        assert np.array_equal(a[k], b[k]), k
