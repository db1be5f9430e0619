"""-m gpu: bench.py as the driver runs it - one JSON line with the contract's keys, sane values; --full with everything else the
line can carry; --dump-outputs: the last timed step's outputs, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), *args], text=True, cwd=ROOT, timeout=600)
    lines = [l for l in out.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_bench_line_contract():
    d = _run("--gpus", "1", "--steps", "6", "--warmup", "2", "--cpu-seconds", "1.0", "--full")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "also"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    # value is whole-job keyword-steps/s: units / time
    assert d["value"] == pytest.approx(4096 * 256 * 6 / (d["ms_per_step"] * 6e-3), rel=1e-6)
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"]) and 0 < r["frac"] < 1
    assert r["achieved"] == pytest.approx(r["algorithmic_bytes_per_launch"] / (r["kernel_ms"] * 1e-3) / 1e9, rel=1e-9)
    assert r["algorithmic_bytes_per_launch"] == 4096 * 256 * 56 + 26 * 4096 and r["launches"] == 6
    _kernel_time_fits_the_step(d)
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "sample" in c
    assert c["single_thread"]["cores"] == 1 and 0 < c["single_thread"]["value"] <= c["value"] * 1.5
    assert c["reference_python"]["value"] > 0 and "provenance" in c["reference_python"]
    assert d["value"] > 100 * c["value"]
    assert 0 < d["episode_metric"]["NCP"] < 2
    if r["traffic"] is not None:
        assert r["traffic_source"]                      # a number not measured in this process says where it is from
    # the largest single-GPU config and the per-GPU shards of the 8-GPU configs, measured in the same run
    a = d["also"]
    assert set(a) == {"cfg3", "cfg4", "cfg5"}
    assert a["cfg3"]["steps"] >= 50 and a["cfg3"]["roofline"]["algorithmic_bytes_per_launch"] == 16384 * 1024 * 56 + 26 * 16384
    assert a["cfg3"]["value"] == pytest.approx(16384 * 1024 / (a["cfg3"]["ms_per_step"] * 1e-3), rel=1e-6)
    assert a["cfg3"]["roofline"]["frac"] > d["roofline"]["frac"]          # the sparse config is the HBM-heavy one


def _kernel_time_fits_the_step(d):
    """the kernel time (untimed pass of the same length, the batch as one launch) cannot exceed the time of a step scheduled the same
    way by more than noise; a step run as env groups on several streams may be shorter than that, and the line says so"""
    r, g = d["roofline"], d["env_groups"]
    assert g["profiled_pass"] == 1 and r["envs_per_launch"]["timed_region"] * g["timed_region"] == r["envs_per_launch"]["profiled_pass"]
    assert r["launches_in_timed_region"] == (d["steps"] if g["timed_region"] == 1 else 1 + (d["steps"] - 1) * g["timed_region"])
    if g["timed_region"] == 1:
        assert r["kernel_ms"] <= d["ms_per_step"] * 1.05
    else:
        assert r["kernel_ms"] <= g["ms_per_step_as_one_group"] * 1.05
        assert d["ms_per_step"] <= g["ms_per_step_as_one_group"] * 1.05 and "BELOW" in g["note"]


def test_driver_shaped_run_times_a_region_without_event_records():
    """what the driver runs (--steps 20 --warmup 5): exactly 20 launches in the timed region, no event record among them; the
    kernel time comes from the separate, untimed, equally long pass and cannot exceed the step time by more than noise"""
    d = _run("--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-also", "--full")
    r = d["roofline"]
    assert d["steps"] == 20 and d["warmup"] == 5
    assert r["launches_in_timed_region"] == 1 + 19 * d["env_groups"]["timed_region"] and r["event_records_in_timed_region"] == 0 and r["launches"] == 20
    assert "untimed pass" in r["kernel_ms_method"]
    _kernel_time_fits_the_step(d)


def test_bench_other_configs_run():
    d = _run("--config", "cfg5", "--steps", "4", "--warmup", "1", "--no-cpu-baseline", "--full")
    assert "drift True" in d["config"]["workload"] and d["roofline"]["algorithmic_bytes_per_launch"] == 2048 * 1024 * 68 + 26 * 2048
    assert "also" not in d
    d = _run("--budget", "50", "--steps", "4", "--warmup", "2", "--no-cpu-baseline", "--no-also", "--full")
    assert "k_step_exact_rows" in d["roofline"]["kernel"]


def test_bench_two_ranks_on_one_gpu_with_the_stand_in_reduction():
    """`--gpus 2` starts two rank processes; on a one-GPU box both engines share the device, so the reduction goes
    through the file stand-in (RCCL refuses two ranks on one device; the RCCL call itself is covered at world size 1 by
    test_gpu_device_resident.py).  Everything else - sharding by global env id, the per-episode reduction inside the timed
    region, the slowest rank's time, rank 0's line - is the N > 1 path as the driver runs it."""
    env = dict(os.environ, ADCRAFT_DIST_BACKEND="file")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "61", "--warmup", "2",
                                   "--config", "cfg5", "--full"], text=True, cwd=ROOT, timeout=900, env=env)
    d = json.loads([ln for ln in out.strip().splitlines() if ln.startswith("{")][0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak"
    assert d["value"] == pytest.approx(2 * 2048 * 1024 / (d["ms_per_step"] * 1e-3), rel=1e-6)
    assert d["episode_metric"]["env_steps"] == 2 * 2048 * 61


FULL_ONLY = ("roofline", "roofline_valu", "env_groups", "ms_per_step_before_clock_spin", "episode_metric", "cpu_baseline", "also", "host_step")
OUTPUT_NAMES = {"impressions", "buyside_clicks", "sellside_conversions", "cost", "revenue", "reward", "cumulative_profit", "days_passed",
                "terminated", "truncated", "env_index"}


def _outputs(d):
    out = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert set(out) == OUTPUT_NAMES
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
    return out


def _same_outputs(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


def test_plain_run_is_lean_and_dumps_the_same_outputs_every_time(tmp_path):
    """the driver's command does only what the headline needs; the timed steps start from the engine's state after the set-up whatever
    ran before them (the clock spin's length varies from run to run, --full adds three passes), so the dumped outputs are identical"""
    d = _run("--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs", str(tmp_path / "a"))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config"):
        assert k in d, k
    assert not [k for k in FULL_ONLY if k in d]
    assert d["steps"] == 20 and d["warmup"] == 5 and d["higher_is_better"] is True and d["unit"] == "keyword-steps/s"
    assert d["value"] == pytest.approx(4096 * 256 * 20 / (d["ms_per_step"] * 20e-3), rel=1e-6)
    a = _outputs(tmp_path / "a")
    assert a["impressions"].shape == (4096, 256) and a["reward"].shape == (4096,) and a["reward"].dtype == np.float64
    assert np.array_equal(a["env_index"], np.arange(4096)) and a["impressions"].sum() > 0 and a["buyside_clicks"].sum() > 0
    assert (a["days_passed"] == 5 + 20).all()                   # the warm-up and the timed steps, from day 0: the spin left no trace
    _run("--gpus", "1", "--steps", "20", "--warmup", "5", "--spin-seconds", "0", "--dump-outputs", str(tmp_path / "b"))
    _same_outputs(a, _outputs(tmp_path / "b"))
    f = _run("--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--no-cpu-baseline", "--no-also", "--dump-outputs", str(tmp_path / "c"))
    assert "roofline" in f and "episode_metric" in f
    _same_outputs(a, _outputs(tmp_path / "c"))


def test_dumped_outputs_with_drift_binding_budgets_and_a_large_config(tmp_path):
    """the restore before the warm-up also undoes drift (parameters, pending updates) and the budget-exact paths' state; outputs larger
    than 64 MB are dumped as a fixed sample of env rows"""
    for name, args in (("drift", ("--config", "cfg5")), ("budget", ("--budget", "50"))):
        for spin in ("0", "0.2"):
            _run("--steps", "7", "--warmup", "3", "--spin-seconds", spin, *args, "--dump-outputs", str(tmp_path / f"{name}_{spin}"))
        x = _outputs(tmp_path / f"{name}_0")
        _same_outputs(x, _outputs(tmp_path / f"{name}_0.2"))
        assert (x["days_passed"] == 10).all()
    _run("--config", "cfg3", "--steps", "2", "--warmup", "1", "--spin-seconds", "0", "--dump-outputs", str(tmp_path / "cfg3"))
    s = _outputs(tmp_path / "cfg3")
    rows = s["env_index"].astype(np.int64)
    assert 1000 < len(rows) < 16384 and (np.diff(rows) > 0).all() and rows[-1] < 16384
    assert s["impressions"].shape == (len(rows), 1024) and s["reward"].shape == (len(rows),) and (s["days_passed"] == 3).all()
