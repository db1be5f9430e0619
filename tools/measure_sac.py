#!/usr/bin/env python3
"""Soft actor-critic on the device, measured (profiles/pr_sac_trainer.txt).  Every measurement is a child process of its own
under a time limit; the parent process never opens the GPU, and the first child that fails ends the run.

  update   ms of one sac_update and of a call of 64 updates per update; host clock around synchronised calls, after an untimed
           round.  Next to it, in the same child, this build's own td3_update with policy_delay 1 (an actor step in every
           update) at the same shape: the second yardstick
  torch    the same SAC update in PyTorch on the same GPU: a resident buffer of the same size, index gather, the soft target
           under the live actor, both critics' loss, the actor's step through min(Q1, Q2), the temperature's step, Polyak,
           torch.optim.Adam, float32 autograd: the first yardstick
  waits    set-up, one update and then one no-clip call of --waits-updates updates, alone in a process: run it under a HIP-API
           trace with 64 and with 0; the difference of the synchronising calls is what the call of 64 waits for
  parent   with --parent-tree (a checkout of the parent commit, its library built): bench.py, the single-policy
           run_days("mlp") day, solo td3_update and pg_minibatch of the parent and of this checkout, alternating, their
           run-to-run spread, and bench.py --dump-outputs of both compared byte for byte (tools/measure_td3.py's and
           tools/measure_pg.py's children, each run from its own tree)

    python tools/measure_sac.py [--shapes 1024x25,4096x256] [--critics 32,32;256,256] [--batches 256,2048] [--reps 5]
                                [--parent-tree DIR [--rounds 3]]
Kernel shares of an update: rocprofv3 --kernel-trace --stats -- python tools/measure_sac.py --child update --shape 4096x256
--critic 256,256 --batch 256 (a run of its own).
"""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))
from measure_td3 import DAYS, parent as td3_parent, report, timed  # noqa: E402


def td3_trainer(N, K, critic, batch, **kw):
    """tools/measure_td3.py's trainer with further options of the preset"""
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    from adcraft_amd.baselines.es_trainer import default_policy
    from adcraft_amd.baselines.td3_trainer import TD3Trainer, td3
    e = eng.StepEngine(N, K, seed=7, max_days=DAYS)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    cfg = td3(critic_hidden=critic, batch_size=batch, capacity=4 * DAYS * N, learning_starts=1 << 40, reward_scale=0.1, seed=3, **kw)
    return e, TD3Trainer(e, default_policy(K, hidden=(32, 32), days=DAYS), horizon=DAYS, **cfg)


def sac_policy(K):
    from adcraft_amd.baselines.es_trainer import default_policy
    from adcraft_amd.baselines.mlp_policy import MLPPolicy
    base = default_policy(K, hidden=(32, 32), days=DAYS)
    rng, A = np.random.default_rng(0), K + 1
    w, b = base.layers[-1]
    last = (np.concatenate([w, (rng.standard_normal(w.shape) * 0.01).astype(np.float32)], axis=1),
            np.concatenate([np.zeros(A, np.float32), np.full(A, -1.0, np.float32)]))
    return MLPPolicy(list(base.layers[:-1]) + [last], activation="tanh", shift=base.shift, scale=base.scale, log_std_clamp=(-5.0, 1.0))


def trainer(N, K, critic, batch):
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    from adcraft_amd.baselines.sac_trainer import SACTrainer, sac
    e = eng.StepEngine(N, K, seed=7, max_days=DAYS)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    cfg = sac(K, critic_hidden=critic, batch_size=batch, capacity=4 * DAYS * N, learning_starts=1 << 40, reward_scale=0.1, seed=3)
    lo, hi = np.full(K + 1, 0.01, np.float32), np.full(K + 1, 3.0, np.float32)
    return e, SACTrainer(e, sac_policy(K), lo, hi, horizon=DAYS, **cfg)


def child_update(a, N, K, critic):
    e, tr = trainer(N, K, critic, a.batch)
    rows = {k: [] for k in ("sac store per day", "sac update", "sac per update/64")}
    for rep in range(a.reps + 1):
        e.reset()
        e.rollout_reset()
        e.run_days("mlp", DAYS, 100000.0)
        t = {"sac store per day": timed(e.sac_store, e.synchronize) / DAYS, "sac update": timed(lambda: e.sac_update(1), e.synchronize),
             "sac per update/64": timed(lambda: e.sac_update(64), e.synchronize) / 64}
        if rep:
            for k, v in t.items():
                rows[k].append(v)
    size = e.sac_buffer(fetch=False)["size"]
    e.close()
    # the second yardstick: this build's TD3 with an actor step in every update
    e, _ = td3_trainer(N, K, critic, a.batch, policy_delay=1)
    rows.update({k: [] for k in ("td3 update", "td3 per update/64")})
    for rep in range(a.reps + 1):
        e.reset()
        e.rollout_reset()
        e.run_days("mlp", DAYS, 100000.0)
        e.td3_store()
        t = {"td3 update": timed(lambda: e.td3_update(1), e.synchronize), "td3 per update/64": timed(lambda: e.td3_update(64), e.synchronize) / 64}
        if rep:
            for k, v in t.items():
                rows[k].append(v)
    e.close()
    print(f"update {N} x {K} (D {5 * K + 2}, A {K + 1}) critics {critic} batch {a.batch}, ring of {size} transitions, actor (32, 32); td3: policy_delay 1")
    report(rows)
    print(f"  sac / td3 (medians): one update {np.median(rows['sac update']) / np.median(rows['td3 update']):.3f}, "
          f"per update of 64 {np.median(rows['sac per update/64']) / np.median(rows['td3 per update/64']):.3f}", flush=True)


def child_torch(a, N, K, critic):
    import torch
    e, tr = trainer(N, K, critic, a.batch)
    e.run_days("mlp", DAYS, 100000.0)
    e.sac_store()
    buf = e.sac_buffer()
    pol = tr.policy().policy
    from adcraft_amd.baselines.td3_trainer import random_critics
    crit = random_critics(K, critic, 0)
    e.close()
    dev, A = torch.device("cuda"), K + 1
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float32, device=dev)
    X, U_, R_, X2, DN = t(buf["x"]), t(buf["a"]), t(buf["r"]), t(buf["x2"]), t(buf["done"].astype(np.float32))
    net = lambda layers, grad: [(t(w).requires_grad_(grad), t(b).requires_grad_(grad)) for w, b in layers]
    actor = net(pol.layers, True)
    qs, qs_t = [net(c, True) for c in crit], [net(c, False) for c in crit]
    log_alpha = torch.zeros((), device=dev, requires_grad=True)
    flat = lambda nets: [p for n in nets for l in n for p in l]
    opt_a, opt_c, opt_t = torch.optim.Adam(flat([actor]), lr=3e-4), torch.optim.Adam(flat(qs), lr=3e-4), torch.optim.Adam([log_alpha], lr=3e-4)

    def forward(ls, x):
        for i, (w, b) in enumerate(ls):
            x = x @ w + b
            if i + 1 < len(ls):
                x = torch.tanh(x)
        return x

    def sample(x):
        o = forward(actor, x)
        ls = torch.clamp(o[:, A:], -5.0, 1.0)
        z = torch.randn_like(ls)
        tt = torch.tanh(o[:, :A] + torch.exp(ls) * z)
        lp = (-0.5 * z * z - ls).sum(dim=1) - A * 0.9189385 - torch.log(1 - tt * tt + 1e-6).sum(dim=1)
        return tt, lp

    def update():
        idx = torch.randint(0, X.shape[0], (a.batch,), device=dev)
        x, u, r, x2, dn = X[idx], U_[idx], R_[idx], X2[idx], DN[idx]
        alpha = log_alpha.exp().detach()
        with torch.no_grad():
            t2, lp2 = sample(x2)
            row2 = torch.cat([x2, t2], dim=1)
            y = 0.1 * r + 0.99 * (1 - dn) * (torch.minimum(forward(qs_t[0], row2)[:, 0], forward(qs_t[1], row2)[:, 0]) - alpha * lp2)
        row = torch.cat([x, torch.tanh(u)], dim=1)
        loss = sum((0.5 * (forward(q, row)[:, 0] - y) ** 2).mean() for q in qs)
        opt_c.zero_grad(set_to_none=True)
        loss.backward()
        opt_c.step()
        tt, lp = sample(x)
        rowp = torch.cat([x, tt], dim=1)
        la = (alpha * lp - torch.minimum(forward(qs[0], rowp)[:, 0], forward(qs[1], rowp)[:, 0])).mean()
        opt_a.zero_grad(set_to_none=True)
        la.backward()
        opt_a.step()
        lt = -(log_alpha * (lp.detach().mean() - float(A)))
        opt_t.zero_grad(set_to_none=True)
        lt.backward()
        opt_t.step()
        with torch.no_grad():
            torch._foreach_lerp_(flat(qs_t), flat(qs), 0.005)

    rows = {k: [] for k in ("torch update", "torch per update/64")}
    for rep in range(a.reps + 1):
        tt = {"torch update": timed(update, torch.cuda.synchronize), "torch per update/64": timed(lambda: [update() for _ in range(64)], torch.cuda.synchronize) / 64}
        if rep:
            for k, v in tt.items():
                rows[k].append(v)
    print(f"torch  {N} x {K} critics {critic} batch {a.batch} (float32 autograd, resident buffer and parameters, torch.optim.Adam)")
    report(rows)


def child_waits(a, N, K, critic):
    """set-up and one update, then one no-clip call of --waits-updates updates (0: none).  Trace it twice, with 64 and with 0: the
    difference of the two traces' synchronising HIP calls is what the call of 64 waits for"""
    e, tr = trainer(N, K, critic, a.batch)
    e.run_days("mlp", DAYS, 100000.0)
    e.sac_store()
    e.sac_update(1)
    e.synchronize()
    if a.waits_updates:
        e.sac_update(a.waits_updates)
    print(f"measure_sac: waits child ran sac_update({a.waits_updates})" if a.waits_updates else "measure_sac: waits child ran no further update", flush=True)
    e.close()


def parent(a):
    """bench.py and the single-policy day (measure_td3's), then solo td3_update and pg_minibatch, each from its own tree, alternating"""
    td3_parent(a)
    trees = dict(parent=os.path.abspath(a.parent_tree), this=HERE)
    for _ in range(a.rounds):
        for label, tree in trees.items():
            env = dict(os.environ, ADCRAFT_HIP_LIB=os.path.join(tree, "adcraft_amd", "lib", "libadcraft_hip.so"))
            for tool, extra in (("measure_td3.py", ["--critic", "256,256", "--batch", "256"]), ("measure_pg.py", [])):
                print(f"[{label}] {tool} --child update --shape 4096x256", flush=True)
                rc = subprocess.run([sys.executable, os.path.join(tree, "tools", tool), "--child", "update", "--shape", "4096x256", "--reps", "3"] + extra,
                                    cwd=tree, env=env, timeout=a.child_timeout).returncode
                if rc != 0:
                    sys.exit(f"measure_sac: {tool} of {label} ended with status {rc}; stopping")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x25,4096x256")
    ap.add_argument("--critics", default="32,32;256,256")
    ap.add_argument("--batches", default="256,2048")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", default=None, choices=["update", "torch", "waits"])
    ap.add_argument("--shape", default="4096x256")
    ap.add_argument("--critic", default="256,256")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--waits-updates", type=int, default=64)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3, help="parent / this alternations")
    a = ap.parse_args()
    if a.child:
        N, K = (int(x) for x in a.shape.split("x"))
        critic = tuple(int(x) for x in a.critic.split(","))
        return dict(update=child_update, torch=child_torch, waits=child_waits)[a.child](a, N, K, critic)
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
                        sys.exit(f"measure_sac: child {what} {shape} {critic} {batch} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
