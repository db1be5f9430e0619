#!/usr/bin/env python3
"""Off-policy (TD3) training on the device, measured (profiles/pr_td3_trainer.txt).  Every measurement is a child process of its
own under a time limit; the parent process never opens the GPU, and the first child that fails ends the run.

  update   ms of td3_store per recorded day, of one td3_update without an actor step and of one with (policy_delay 2: the odd
           and the even update), and of a call of 64 updates per update; host clock around synchronised calls, after an untimed
           round
  torch    the same update in PyTorch on the same GPU: a resident buffer of the same size, index gather, target actor and
           critics, both critics' loss, the delayed actor step, Polyak, torch.optim.Adam, float32 autograd

  parent   with --parent-tree (a checkout of the parent commit, its library built): bench.py and the single-policy
           run_days("mlp") day (tools/measure_es.py --child day) of the parent and of this checkout, alternating, their
           run-to-run spread, and bench.py --dump-outputs of both compared byte for byte

    python tools/measure_td3.py [--shapes 1024x25,4096x256] [--critics 32,32;256,256] [--batches 256,2048] [--reps 5]
                                [--parent-tree DIR [--rounds 3]]
Kernel shares of an update: rocprofv3 --kernel-trace --stats -- python tools/measure_td3.py --child update --shape 4096x256
--critic 256,256 --batch 256 (a run of its own; counters, if any, in another run without tracing).
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
DAYS = 10


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def trainer(N, K, critic, batch):
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    from adcraft_amd.baselines.es_trainer import default_policy
    from adcraft_amd.baselines.td3_trainer import TD3Trainer, td3
    e = eng.StepEngine(N, K, seed=7, max_days=DAYS)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    cfg = td3(critic_hidden=critic, batch_size=batch, capacity=4 * DAYS * N, learning_starts=1 << 40, reward_scale=0.1, seed=3)
    return e, TD3Trainer(e, default_policy(K, hidden=(32, 32), days=DAYS), horizon=DAYS, **cfg)


def report(rows):
    for k, v in rows.items():
        print(f"  {k:16s} ms " + " ".join(f"{x:9.4f}" for x in v) + f"   (min {min(v):.4f}, median {np.median(v):.4f})", flush=True)


def child_update(a, N, K, critic):
    e, tr = trainer(N, K, critic, a.batch)
    rows = {k: [] for k in ("store per day", "update", "update + actor", "per update of 64")}
    for rep in range(a.reps + 1):
        e.reset()
        e.rollout_reset()
        e.run_days("mlp", DAYS, 100000.0)
        t = {"store per day": timed(e.td3_store, e.synchronize) / DAYS}
        if e.td3_state()["updates"] % 2:
            e.td3_update(1)
        t["update"] = timed(lambda: e.td3_update(1), e.synchronize)
        t["update + actor"] = timed(lambda: e.td3_update(1), e.synchronize)
        t["per update of 64"] = timed(lambda: e.td3_update(64), e.synchronize) / 64
        if rep:
            for k, v in t.items():
                rows[k].append(v)
    size = e.td3_buffer(fetch=False)["size"]
    e.close()
    print(f"update {N} x {K} (D {5 * K + 2}, A {K + 1}) critics {critic} batch {a.batch}, ring of {size} transitions, actor (32, 32)")
    report(rows)


def child_torch(a, N, K, critic):
    import torch
    e, tr = trainer(N, K, critic, a.batch)
    e.run_days("mlp", DAYS, 100000.0)
    e.td3_store()
    buf = e.td3_buffer()
    pol = tr.policy()
    from adcraft_amd.baselines.td3_trainer import random_critics
    crit = random_critics(K, critic, 0)
    e.close()
    dev = torch.device("cuda")
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float32, device=dev)
    X, A_, R_, X2, DN = t(buf["x"]), t(buf["a"]), t(buf["r"]), t(buf["x2"]), t(buf["done"].astype(np.float32))
    net = lambda layers, grad: [(t(w).requires_grad_(grad), t(b).requires_grad_(grad)) for w, b in layers]
    actor, actor_t = net(pol.layers, True), net(pol.layers, False)
    qs, qs_t = [net(c, True) for c in crit], [net(c, False) for c in crit]
    flat = lambda nets: [p for n in nets for l in n for p in l]
    opt_a, opt_c = torch.optim.Adam(flat([actor]), lr=1e-3), torch.optim.Adam(flat(qs), lr=1e-3)

    def forward(ls, x):
        for i, (w, b) in enumerate(ls):
            x = x @ w + b
            if i + 1 < len(ls):
                x = torch.tanh(x)
        return x

    def update(with_actor):
        idx = torch.randint(0, X.shape[0], (a.batch,), device=dev)
        x, ac, r, x2, dn = X[idx], A_[idx], R_[idx], X2[idx], DN[idx]
        with torch.no_grad():
            a2 = forward(actor_t, x2) + torch.clamp(0.2 * torch.randn_like(ac), -0.5, 0.5)
            row2 = torch.cat([x2, a2], dim=1)
            y = 0.1 * r + 0.99 * (1 - dn) * torch.minimum(forward(qs_t[0], row2)[:, 0], forward(qs_t[1], row2)[:, 0])
        row = torch.cat([x, ac], dim=1)
        loss = sum((0.5 * (forward(q, row)[:, 0] - y) ** 2).mean() for q in qs)
        opt_c.zero_grad(set_to_none=True)
        loss.backward()
        opt_c.step()
        if with_actor:
            la = -forward(qs[0], torch.cat([x, forward(actor, x)], dim=1))[:, 0].mean()
            opt_a.zero_grad(set_to_none=True)
            la.backward()
            opt_a.step()
            with torch.no_grad():
                for live, targ in ((flat([actor]), flat([actor_t])), (flat(qs), flat(qs_t))):
                    torch._foreach_lerp_(targ, live, 0.005)

    rows = {k: [] for k in ("update", "update + actor", "per update of 64")}
    for rep in range(a.reps + 1):
        tt = {"update": timed(lambda: update(False), torch.cuda.synchronize), "update + actor": timed(lambda: update(True), torch.cuda.synchronize),
              "per update of 64": timed(lambda: [update(i % 2 == 1) for i in range(64)], torch.cuda.synchronize) / 64}
        if rep:
            for k, v in tt.items():
                rows[k].append(v)
    print(f"torch  {N} x {K} critics {critic} batch {a.batch} (float32 autograd, resident buffer and parameters, torch.optim.Adam)")
    report(rows)


def parent(a):
    """bench.py and the single-policy day, parent / this alternating; the dumped outputs of the two compared"""
    import filecmp
    import json
    import tempfile
    trees = dict(parent=os.path.abspath(a.parent_tree), this=HERE)
    dumps = {k: tempfile.mkdtemp(prefix=f"td3_dump_{k}_") for k in trees}
    ms = {k: [] for k in trees}
    for _ in range(a.rounds):
        for label, tree in trees.items():
            env = dict(os.environ, ADCRAFT_HIP_LIB=os.path.join(tree, "adcraft_amd", "lib", "libadcraft_hip.so"))
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "300", "--warmup", "30", "--dump-outputs", dumps[label]],
                                 cwd=tree, env=env, timeout=a.child_timeout, capture_output=True, text=True)
            if out.returncode != 0:
                sys.exit(f"measure_td3: bench.py of {label} ended with status {out.returncode}; stopping")
            ms[label].append(json.loads(out.stdout.strip().splitlines()[-1])["ms_per_step"])
            rc = subprocess.run([sys.executable, os.path.join(HERE, "tools", "measure_es.py"), "--child", "day", "--shape", "4096x256", "--tree", tree,
                                 "--label", label, "--reps", "3", "--days", "30"], env=env, timeout=a.child_timeout).returncode
            if rc != 0:
                sys.exit(f"measure_td3: the day of {label} ended with status {rc}; stopping")
    for label in trees:
        v = ms[label]
        print(f"bench.py ms_per_step {label:6s}: " + " ".join(f"{x:.4f}" for x in v) + f"  (min {min(v):.4f}, spread {max(v) - min(v):.4f})")
    names = sorted(os.listdir(dumps["this"]))
    same = [n for n in names if filecmp.cmp(os.path.join(dumps["this"], n), os.path.join(dumps["parent"], n), shallow=False)]
    print(f"bench.py --dump-outputs: {len(same)} of {len(names)} files byte-identical to the parent's"
          + ("" if len(same) == len(names) else f"; DIFFERENT: {sorted(set(names) - set(same))}"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x25,4096x256")
    ap.add_argument("--critics", default="32,32;256,256")
    ap.add_argument("--batches", default="256,2048")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", default=None, choices=["update", "torch"])
    ap.add_argument("--shape", default="4096x256")
    ap.add_argument("--critic", default="256,256")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3, help="parent / this alternations")
    a = ap.parse_args()
    if a.child:
        N, K = (int(x) for x in a.shape.split("x"))
        critic = tuple(int(x) for x in a.critic.split(","))
        return (child_update if a.child == "update" else child_torch)(a, N, K, critic)
    if a.parent_tree:
        return parent(a)
    for shape in a.shapes.split(","):
        for critic in a.critics.split(";"):
            for batch in a.batches.split(","):
                for what in ("update", "torch"):
                    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--shape", shape, "--critic", critic, "--batch", batch,
                           "--reps", str(a.reps)]
                    rc = subprocess.run(cmd, timeout=a.child_timeout).returncode        # (a timeout raises: nothing more is started)
                    if rc != 0:
                        sys.exit(f"measure_td3: child {what} {shape} {critic} {batch} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
