#!/usr/bin/env python3
"""DevicePPOTrainer.ppo_update with the networks as one call each, on one MI355X -> profiles/net_train_bench.txt ("The
networks as one call").

For each (N chunks, T) shape of tools/diag/ppo_update_bench.py and both head sets ([3, 5, 3] + [2, 2, 2, 2] with use_prior at width
21; [41, 41, 41, 30] at width 15) the tests' restatement of the reference's policy (tests/net_train_util.py) is timed through
DevicePPOTrainer.ppo_update in two forms that alternate call by call within a run:

parent   the three layer swaps (use_device_mlp, use_device_gru_layer, use_device_act): one autograd function per layer, value_out and
         the prior in eager torch;
new      use_device_networks: one autograd function and one C call per network and direction.

Each run reports the median wall time per call (a host clock around the call and a synchronise); --runs consecutive runs are taken so
the run-to-run spread is on the page, and the last column is the margin per run, (parent - new) / parent. Every shape is measured
without and with base.feature_norm. The outputs of the two legs are checked against each other before anything is timed.

    python tools/diag/net_train_bench.py [--reps 20] [--runs 3] [--out profiles/net_train_bench.txt] [--shapes 320x60,2400x8] [--rev HEAD's name]

The new kernels' own times come from a kernel trace in a run of its own (tracing slows the host): --trace runs a few updates of the
new leg and nothing else, and --summarise turns the trace's database into profiles/net_train_kernel_times.txt:

    rocprofv3 --kernel-trace -d <dir> -o net -- python tools/diag/net_train_bench.py --trace
    python tools/diag/net_train_bench.py --summarise <dir>/net_results.db [--out profiles/net_train_kernel_times.txt]
"""
import argparse
import copy
import os
import subprocess
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aircombat_selfplay_amd as pkg  # noqa: E402
import net_train_util as NU  # noqa: E402  (the tests' restatement of the reference's policy)
import ppo_update_util as PU  # noqa: E402

SHAPES = [(320, 60), (2400, 8), (4096, 60), (16384, 8)]
DONE = 0.02


def ppo_form(pol):
    return types.SimpleNamespace(actor=pol.actor, critic=pol.critic, optimizer=pol.optimizer,
                                 evaluate_actions=lambda obs, ra, rc, a, m: pol.evaluate_actions(obs, obs, ra, rc, a, m))


def sample_for(N, T, heads, g):
    nvec, ns, width = NU.HEADS[heads]
    M = N * T
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    obs = rn(M, width)
    act = torch.stack([torch.randint(0, n, (M,), device="cuda", generator=g) for n in list(nvec) + [2] * ns], -1).float()
    masks = (torch.rand(M, 1, device="cuda", generator=g) > DONE).float()
    return (obs, act, masks, -2.0 + 0.1 * rn(M, 1), rn(M, 1), rn(M, 1), rn(M, 1), rn(N, 1, 128), rn(N, 1, 128))


def legs_for(heads, fnorm):
    base = NU.Policy(heads, fnorm, seed=3)
    parent, new = copy.deepcopy(base), copy.deepcopy(base)
    assert pkg.use_device_mlp(parent) == 4 and pkg.use_device_gru_layer(parent) == 2 and pkg.use_device_act(parent) == 1
    assert pkg.use_device_networks(new) == 2
    return ppo_form(parent), ppo_form(new)


def wall(fns, reps, warm=3):
    """Median wall ms per call of each function, the functions alternating call by call."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ms[i].append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(m)) for m in ms]


def summarise(db_path, out):
    """The new kernels' times from the kernel trace of a --trace run (rocprofv3's sqlite output), one row per kernel and grid."""
    import re
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, grid_x / workgroup_x, count(*), min(duration) / 1e3, avg(duration) / 1e3, max(duration) / 1e3 from kernels "
                      "where name like '%nett::%' group by name, grid_x order by name, grid_x").fetchall()
    total = db.execute("select count(*), sum(duration) / 1e6 from kernels").fetchone()
    new = db.execute("select count(*), sum(duration) / 1e6 from kernels where name like '%nett::%'").fetchone()
    lines = ["# tools/diag/net_train_bench.py --summarise: the kernels of csrc/net_train.hpp in a rocprofv3 --kernel-trace of `net_train_bench.py --trace` (the new",
             "# leg only, feature_norm on, 5 updates per shape and head set, the four shapes 320 x 60, 2400 x 8, 4096 x 60, 16384 x 8); us per launch, grouped",
             "# by the launch's workgroups: 300 is the two small shapes (19 200 rows), 512 / 256 the capped grids of the two large ones, forward / backward",
             f"{'kernel':34s} {'workgroups':>10s} {'launches':>8s} {'min':>8s} {'mean':>8s} {'max':>8s}"]
    for name, wgs, n, lo, mean, hi in rows:
        lines.append(f"{re.sub(r'[(].*', '', name.replace('void ', '')):34s} {wgs:10d} {n:8d} {lo:8.1f} {mean:8.1f} {hi:8.1f}")
    lines.append(f"# all kernels of the traced run: {total[0]} launches, {total[1]:.1f} ms; the new kernels: {new[0]} launches, {new[1]:.2f} ms "
                 f"({100 * new[1] / total[1]:.1f}% of the kernel time)")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--shapes", default="")
    ap.add_argument("--rev", default="", help="the parent commit's name, where the tree that runs is not a git checkout")
    ap.add_argument("--summarise", default="", help="a rocprofv3 kernel-trace database of a --trace run: write the new kernels' times")
    ap.add_argument("--trace", action="store_true", help="a few updates of the new leg per shape and nothing else: for a kernel trace")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise, a.out or os.path.join(ROOT, "profiles", "net_train_kernel_times.txt"))
    a.out = a.out or os.path.join(ROOT, "profiles", "net_train_bench.txt")
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")] if a.shapes else SHAPES
    trainer = pkg.DevicePPOTrainer(PU.trainer_args(), torch.device("cuda", 0))
    if a.trace:
        for N, T in shapes:
            for heads in NU.HEADS:
                _, new = legs_for(heads, True)   # with feature_norm, so that all three new kernels are in the trace
                sample = sample_for(N, T, heads, torch.Generator(device="cuda").manual_seed(1))
                for _ in range(5):
                    trainer.ppo_update(new, sample)
                torch.cuda.synchronize()
        return
    lines = [f"# tools/diag/net_train_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}: DevicePPOTrainer.ppo_update, median wall ms "
             f"of {a.reps} calls per run (a host clock around the call and a synchronise), {a.runs} consecutive runs, the two legs alternating "
             f"call by call; margin = (parent - new) / parent per run"]
    rev = a.rev
    try:
        rev = rev or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        pass
    if rev:
        lines.append(f"# parent commit {rev} plus the working tree of this change")
    lines.append(f"{'N':>6} {'T':>3} {'fnorm':>5} {'heads':28s} " + " ".join(f"{'parent' + str(r + 1):>8} {'new' + str(r + 1):>8}" for r in range(a.runs)) + "  margin per run")
    for N, T, fnorm, heads in [(N, T, f, h) for f in (False, True) for N, T in shapes for h in NU.HEADS]:
        if True:
            nvec, ns, _ = NU.HEADS[heads]
            parent, new = legs_for(heads, fnorm)
            sample = sample_for(N, T, heads, torch.Generator(device="cuda").manual_seed(1))
            # the same update: without feature_norm the actor's kernels and arguments are the same, so its parameters are the same
            # bits; value_out and feature_norm are eager torch in the parent leg and kernels in the new one
            six_p, six_n = trainer.ppo_update(parent, sample), trainer.ppo_update(new, sample)
            assert all(torch.allclose(x, y, rtol=1e-4, atol=1e-6) for x, y in zip(six_p, six_n)), (N, T, heads, six_p, six_n)
            same = torch.equal if not fnorm else (lambda p, q: torch.allclose(p, q, rtol=1e-4, atol=1e-5))
            assert all(same(p, q) for p, q in zip(parent.actor.parameters(), new.actor.parameters())), (N, T, heads)
            reps = max(5, a.reps // 2) if N * T > 100000 else a.reps
            runs = [wall([lambda: trainer.ppo_update(parent, sample), lambda: trainer.ppo_update(new, sample)], reps) for _ in range(a.runs)]
            name = str(list(nvec)) + (f" + {[2] * ns}" if ns else "")
            lines.append(f"{N:6d} {T:3d} {'on' if fnorm else 'off':>5} {name:28s} " + " ".join(f"{p:8.3f} {n:8.3f}" for p, n in runs) + "  " +
                         " ".join(f"{100 * (p - n) / p:+5.1f}%" for p, n in runs))
            print(lines[-1], flush=True)
            del parent, new, sample
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
