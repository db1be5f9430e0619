#!/usr/bin/env python3
"""Policy-gradient training on the device, measured (profiles/pr_pg_trainer.txt).  Every measurement is a child process of its
own under a time limit; the parent process never opens the GPU, and the first child that fails ends the run.

  update   ms of pg_advantages, of one pg_minibatch and of a full pg_update (epochs x minibatches) on a record of T days, and
           of the collection of those T days (run_days("mlp")); host clock around synchronised calls, after an untimed round
  torch    the same update in PyTorch on the same GPU: the record's arrays already resident as device tensors, float32
           autograd, the same minibatching (env ranges, whole trajectories), torch.optim.Adam, the same loss

  parent   with --parent-tree (a checkout of the parent commit, its library built): bench.py and the single-policy
           run_days("mlp") day (tools/measure_es.py --child day) of the parent and of this checkout, alternating, and
           bench.py --dump-outputs of both compared byte for byte

    python tools/measure_pg.py [--shapes 4096x256,1024x25] [--hidden 64,64] [--days 60] [--epochs 4] [--minibatches 4] [--reps 5]
                               [--parent-tree DIR [--rounds 3]]
Kernel times of a minibatch: rocprofv3 --kernel-trace --stats -- python tools/measure_pg.py --child update --shape 4096x256
(a run of its own).
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def policy(K, hidden, days):
    from adcraft_amd.baselines.es_trainer import default_policy
    pol = default_policy(K, hidden=hidden, days=days, seed=0)
    rng = np.random.default_rng(1)
    layers, n_in = [], 5 * K + 2
    for n_out in list(hidden) + [1]:
        b = 1.0 / np.sqrt(n_in)
        layers.append((rng.uniform(-b, b, (n_in, n_out)).astype(np.float32), rng.uniform(-b, b, n_out).astype(np.float32)))
        n_in = n_out
    pol.value_layers = layers
    return pol


def collect(N, K, hidden, days, cfg):
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    e = eng.StepEngine(N, K, seed=7, max_days=days)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    pol = policy(K, hidden, days)
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(days, obs=True)
    e.pg_init(**cfg)
    return e, pol


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def child_update(a, N, K, hidden):
    cfg = dict(lr=3e-4, minibatch_envs=N // a.minibatches)
    e, _ = collect(N, K, hidden, a.days, cfg)
    rows = {k: [] for k in ("collect", "advantages", "minibatch", "update")}
    for rep in range(a.reps + 1):
        e.reset()
        e.rollout_reset()
        t = dict(collect=timed(lambda: e.run_days("mlp", a.days, 100000.0), e.synchronize),
                 advantages=timed(e.pg_advantages, e.synchronize),
                 minibatch=timed(lambda: e.pg_minibatch(0, N // a.minibatches), e.synchronize),
                 update=timed(lambda: e.pg_update(a.epochs), e.synchronize))
        if rep:
            for k, v in t.items():
                rows[k].append(v)
    e.close()
    D = 5 * K + 2
    print(f"update {N} x {K} hidden {hidden} T {a.days}, {a.epochs} epochs x {a.minibatches} minibatches "
          f"(record {a.days * N * (D + K + 6) * 4 / 1e6:.1f} MB, what a fetch / upload trainer would move per iteration)")
    for k, v in rows.items():
        print(f"  {k:11s} ms " + " ".join(f"{x:9.3f}" for x in v) + f"   (min {min(v):.3f}, median {np.median(v):.3f})", flush=True)


def child_torch(a, N, K, hidden):
    import torch
    cfg = dict(lr=3e-4, minibatch_envs=N // a.minibatches)
    e, pol = collect(N, K, hidden, a.days, cfg)
    e.run_days("mlp", a.days, 100000.0)
    rec = e.rollout_fetch()
    adv, ret = e.pg_advantages(fetch=True)
    e.close()
    dev = torch.device("cuda")
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float32, device=dev)
    obs, act, logp_old, advt, rett = t(rec["obs"]), t(rec["action"]), t(rec["logp"]), t(adv), t(ret)
    A = K + 1

    def net(layers):
        return [(t(w).requires_grad_(), t(b).requires_grad_()) for w, b in layers]
    pl, vl = net(pol.layers), net(pol.value_layers)
    log_std = t(pol.log_std).requires_grad_()
    params = [p for l in pl + vl for p in l] + [log_std]
    opt = torch.optim.Adam(params, lr=3e-4)

    def forward(ls, x):
        for i, (w, b) in enumerate(ls):
            x = x @ w + b
            if i + 1 < len(ls):
                x = torch.tanh(x)
        return x

    def minibatch(n0, B):
        sl = slice(n0, n0 + B)
        x = obs[:, sl].reshape(-1, obs.shape[-1])
        mean = forward(pl, x)
        z = (act[:, sl].reshape(-1, A) - mean) / torch.exp(log_std)
        logp = (-0.5 * z * z - log_std).sum(dim=1) - A * 0.9189385332
        ratio = torch.exp(logp - logp_old[:, sl].reshape(-1))
        ad = advt[:, sl].reshape(-1)
        loss = -torch.minimum(ratio * ad, torch.clamp(ratio, 0.8, 1.2) * ad).mean()
        loss = loss + 0.5 * 0.5 * ((forward(vl, x)[:, 0] - rett[:, sl].reshape(-1)) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 0.5)
        opt.step()

    mb = N // a.minibatches
    rows = dict(minibatch=[], update=[])
    for rep in range(a.reps + 1):
        one = timed(lambda: minibatch(0, mb), torch.cuda.synchronize)
        upd = timed(lambda: [minibatch(i * mb, mb) for _ in range(a.epochs) for i in range(a.minibatches)], torch.cuda.synchronize)
        if rep:
            rows["minibatch"].append(one)
            rows["update"].append(upd)
    print(f"torch  {N} x {K} hidden {hidden} T {a.days}, {a.epochs} epochs x {a.minibatches} minibatches (float32 autograd, resident tensors)")
    for k, v in rows.items():
        print(f"  {k:11s} ms " + " ".join(f"{x:9.3f}" for x in v) + f"   (min {min(v):.3f}, median {np.median(v):.3f})", flush=True)


def parent(a):
    """bench.py and the single-policy day, parent / this alternating; the dumped outputs of the two compared"""
    import filecmp
    import json
    import tempfile
    trees = dict(parent=os.path.abspath(a.parent_tree), this=HERE)
    dumps = {k: tempfile.mkdtemp(prefix=f"pg_dump_{k}_") for k in trees}
    ms = {k: [] for k in trees}
    for _ in range(a.rounds):
        for label, tree in trees.items():
            env = dict(os.environ, ADCRAFT_HIP_LIB=os.path.join(tree, "adcraft_amd", "lib", "libadcraft_hip.so"))
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "300", "--warmup", "30", "--dump-outputs", dumps[label]],
                                 cwd=tree, env=env, timeout=a.child_timeout, capture_output=True, text=True)
            if out.returncode != 0:
                sys.exit(f"measure_pg: bench.py of {label} ended with status {out.returncode}; stopping")
            ms[label].append(json.loads(out.stdout.strip().splitlines()[-1])["ms_per_step"])
            rc = subprocess.run([sys.executable, os.path.join(HERE, "tools", "measure_es.py"), "--child", "day", "--shape", "4096x256", "--tree", tree,
                                 "--label", label, "--reps", "3", "--days", "30"], env=env, timeout=a.child_timeout).returncode
            if rc != 0:
                sys.exit(f"measure_pg: the day of {label} ended with status {rc}; stopping")
    for label in trees:
        print(f"bench.py ms_per_step {label:6s}: " + " ".join(f"{x:.4f}" for x in ms[label]) + f"  (min {min(ms[label]):.4f})")
    names = sorted(os.listdir(dumps["this"]))
    same = [n for n in names if filecmp.cmp(os.path.join(dumps["this"], n), os.path.join(dumps["parent"], n), shallow=False)]
    print(f"bench.py --dump-outputs: {len(same)} of {len(names)} files byte-identical to the parent's"
          + ("" if len(same) == len(names) else f"; DIFFERENT: {sorted(set(names) - set(same))}"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x256,1024x25")
    ap.add_argument("--hidden", default="64,64;32,32")
    ap.add_argument("--days", type=int, default=60)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", default=None, choices=["update", "torch"])
    ap.add_argument("--shape", default="4096x256")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3, help="parent / this alternations")
    a = ap.parse_args()
    if a.child:
        N, K = (int(x) for x in a.shape.split("x"))
        hidden = tuple(int(x) for x in a.hidden.split(";")[0].split(","))
        return (child_update if a.child == "update" else child_torch)(a, N, K, hidden)
    if a.parent_tree:
        return parent(a)
    for shape in a.shapes.split(","):
        for hidden in a.hidden.split(";"):
            for what in ("update", "torch"):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--shape", shape, "--hidden", hidden, "--days", str(a.days),
                       "--epochs", str(a.epochs), "--minibatches", str(a.minibatches), "--reps", str(a.reps)]
                rc = subprocess.run(cmd, timeout=a.child_timeout).returncode        # (a timeout raises: nothing more is started)
                if rc != 0:
                    sys.exit(f"measure_pg: child {what} {shape} {hidden} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
