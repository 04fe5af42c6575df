#!/usr/bin/env python3
"""Training MLP block timings on one MI355X -> profiles/mlp_train_bench.txt ("The training MLP blocks").

For each (N chunks, T) shape, M = N * T rows: one block (Linear K -> 128, ReLU, LayerNorm) forward under no_grad and forward +
backward, fused (mlp_block) against eager torch on the same GPU, for K = 128 (x takes a gradient) and K = 15 (x is an observation: no
dx); and one whole actor + critic evaluate_actions + loss.backward() minibatch with (a) use_device_gru only, the state before the
fused MLP blocks existed, and (b) use_device_gru and use_device_mlp. The members of each comparison alternate call by call within the
run. Each is reported as the median HIP-event time over the calls and the median wall time per call with a synchronise, after
warm-up. The fused block rows also carry the bytes the block has to move (from the shape: x, y, dy, dx and the row statistics; the
128 x K parameters and the partial sums are left out) and that over the device time as a share of the 8.0 TB/s HBM peak.

    python tools/diag/mlp_train_bench.py [--reps 20] [--out profiles/mlp_train_bench.txt] [--shapes 4096x60,320x60]
"""
import argparse
import copy
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aircombat_selfplay_amd as pkg  # noqa: E402
import mlp_train_util as U  # noqa: E402  (the tests' restatement of the reference's actor / critic, whose layers call self.mlp(x))

SHAPES = [(320, 60), (2400, 8), (4096, 60), (16384, 8)]
DONE = 0.02
HBM_PEAK = 8.0e12


def timed(fns, reps, warm=3):
    """[(device ms, wall ms)] per function, the functions alternating call by call."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)] for _ in range(reps)]
    for e in ev:   # back to back: no host wait between calls
        e[0].record()
        for i, fn in enumerate(fns):
            fn(); e[i + 1].record()
    torch.cuda.synchronize()
    dev = [float(np.median([e[i].elapsed_time(e[i + 1]) for e in ev])) for i in range(len(fns))]
    wall = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); wall[i].append((time.perf_counter() - t0) * 1e3)
    return [(d, float(np.median(w))) for d, w in zip(dev, wall)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_train_bench.txt"))
    ap.add_argument("--shapes", default="")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")] if a.shapes else SHAPES
    torch.manual_seed(0)
    lines = [f"# tools/diag/mlp_train_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, median of {a.reps} (ms): "
             f"device = HIP events over back-to-back calls, wall = per call with a synchronise; MB = what the fused block must move, "
             f"%HBM = MB / device time over {HBM_PEAK / 1e12:.1f} TB/s"]
    try:
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        lines.append(f"# parent commit {rev or '?'} plus the working tree of this change")
    except OSError:
        pass
    lines.append(f"{'N':>6} {'T':>3} {'what':52s} {'device':>9} {'wall':>9} {'MB':>8} {'%HBM':>6}")

    def row(N, T, what, r, nbytes=None):
        tail = f" {nbytes / 1e6:8.1f} {100 * nbytes / (r[0] * 1e-3) / HBM_PEAK:6.1f}" if nbytes else ""
        lines.append(f"{N:6d} {T:3d} {what:52s} {r[0]:9.3f} {r[1]:9.3f}{tail}")
        print(lines[-1], flush=True)

    for N, T in shapes:
        M = N * T
        g = torch.Generator(device="cuda").manual_seed(0)
        for K in (128, 15):
            lin, norm = torch.nn.Linear(K, 128).cuda(), torch.nn.LayerNorm(128).cuda()
            x = torch.randn(M, K, device="cuda", generator=g, requires_grad=(K == 128))
            go = torch.randn(M, 128, device="cuda", generator=g)
            wrt = ([x] if K == 128 else []) + list(lin.parameters()) + list(norm.parameters())
            fused = lambda: pkg.mlp_block(x, lin, norm)
            eager = lambda: norm(torch.relu(lin(x)))

            def fwd(f):
                with torch.no_grad():
                    f()

            def fwdbwd(f):
                torch.autograd.grad(f(), wrt, go)

            r = timed([lambda: fwd(fused), lambda: fwd(eager)], a.reps)
            row(N, T, f"block K = {K}: fused forward (no_grad)", r[0], 4 * M * (K + 128))
            row(N, T, f"block K = {K}: eager forward (no_grad)", r[1])
            r = timed([lambda: fwdbwd(fused), lambda: fwdbwd(eager)], a.reps)
            # forward: x, y, stats; backward: x, dy, stats and dx where x takes a gradient
            row(N, T, f"block K = {K}: fused forward + backward", r[0], 4 * M * ((K + 128 + 2) + (K + 128 + 2) + (K if K == 128 else 0)))
            row(N, T, f"block K = {K}: eager forward + backward", r[1])
            del x, go
        # one whole actor + critic minibatch: evaluate_actions + PPO loss + backward
        g = torch.Generator(device="cuda").manual_seed(1)
        obs = torch.randn(M, U.OBS, device="cuda", generator=g)
        act = torch.stack([torch.randint(0, n, (M,), device="cuda", generator=g) for n in U.NVEC], -1).float()
        ra, rc = torch.randn(N, 1, 128, device="cuda", generator=g), torch.randn(N, 1, 128, device="cuda", generator=g)
        adv, ret = torch.randn(M, 1, device="cuda", generator=g), torch.randn(M, 1, device="cuda", generator=g)
        m = (torch.rand(M, 1, device="cuda", generator=g) > DONE).float()
        pol_gru = U.Policy(seed=3)
        pkg.use_device_gru(pol_gru)
        pol_both = copy.deepcopy(pol_gru)
        assert pkg.use_device_mlp(pol_both) == 4

        def step(pol):
            values, logp, ent = pol.evaluate_actions(obs, obs, ra, rc, act, m)
            ratio = torch.exp(logp - logp.detach())
            loss = -torch.min(ratio * adv, ratio.clamp(0.8, 1.2) * adv).mean() + 0.5 * (values - ret).pow(2).mean() - 0.01 * ent
            pol.optimizer.zero_grad()
            loss.backward()

        r = timed([lambda: step(pol_gru), lambda: step(pol_both)], max(5, a.reps // 2))
        row(N, T, "actor + critic minibatch, fused GRU", r[0])
        row(N, T, "actor + critic minibatch, fused GRU + fused MLP", r[1])
        del obs, act, m, adv, ret
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
