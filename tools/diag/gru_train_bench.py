#!/usr/bin/env python3
"""Training GRU timings on one MI355X -> profiles/gru_train_bench.txt ("The training GRU").

For each (N chunks, T) shape: the fused layer (DeviceGRULayer) forward and forward + backward, the reference-style GRULayer (segment
loop with nonzero().cpu() and nn.GRU, fp32 on the same GPU) at the same done rate and seed, and one whole actor + critic
evaluate_actions + loss.backward() minibatch with and without use_device_gru. Each is reported as the median HIP-event time over
back-to-back calls and the median wall time per call with a synchronise, after warm-up.

    python tools/diag/gru_train_bench.py [--reps 20] [--out profiles/gru_train_bench.txt]
"""
import argparse
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
import test_gpu_gru_train as TG  # noqa: E402  (the tests' restatement of the reference's actor / critic and GRULayer)

SHAPES = [(320, 60), (2400, 8), (4096, 60), (16384, 8)]
DONE = 0.02


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:   # back to back: no host wait between calls (the reference path waits inside, by its nonzero().cpu())
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    dev = float(np.median([a.elapsed_time(b) for a, b in ev]))
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); wall.append((time.perf_counter() - t0) * 1e3)
    return dev, float(np.median(wall))


def layer_inputs(N, T, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(T * N, 128, device="cuda", generator=g, requires_grad=True)
    h = torch.randn(N, 1, 128, device="cuda", generator=g, requires_grad=True)
    m = (torch.rand(T * N, 1, device="cuda", generator=g) > DONE).float()
    go = torch.randn(T * N, 128, device="cuda", generator=g)
    return x, h, m, go


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_train_bench.txt"))
    ap.add_argument("--shapes", default="")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")] if a.shapes else SHAPES
    torch.manual_seed(0)
    lines = [f"# tools/diag/gru_train_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, done rate {DONE}, "
             f"median of {a.reps} (ms): device = HIP events over back-to-back calls, wall = per call with a synchronise"]
    try:
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        lines.append(f"# parent commit {rev or '?'} plus the working tree of this change")
    except OSError:
        pass
    lines.append(f"{'N':>6} {'T':>3} {'what':44s} {'device':>9} {'wall':>9}")

    def row(N, T, what, r):
        lines.append(f"{N:6d} {T:3d} {what:44s} {r[0]:9.3f} {r[1]:9.3f}")
        print(lines[-1], flush=True)

    for N, T in shapes:
        ref = TG.RefGRULayer().cuda()
        holder = torch.nn.Module()
        holder.rnn = TG.RefGRULayer().cuda()
        holder.rnn.load_state_dict(ref.state_dict())
        pkg.use_device_gru(holder)
        dev = holder.rnn
        x, h, m, go = layer_inputs(N, T)

        def fwd(layer):
            with torch.no_grad():
                layer(x, h, m)

        def fwdbwd(layer):
            out, _ = layer(x, h, m)
            (out * go).sum().backward()

        row(N, T, "fused forward (no_grad)", timed(lambda: fwd(dev), a.reps))
        row(N, T, "reference GRULayer forward (no_grad)", timed(lambda: fwd(ref), a.reps))
        row(N, T, "fused forward + backward", timed(lambda: fwdbwd(dev), a.reps))
        row(N, T, "reference GRULayer forward + backward", timed(lambda: fwdbwd(ref), a.reps))
        # one whole actor + critic minibatch: evaluate_actions + PPO loss + backward
        g = torch.Generator(device="cuda").manual_seed(1)
        obs = torch.randn(T * N, TG.OBS, device="cuda", generator=g)
        act = torch.stack([torch.randint(0, n, (T * N,), device="cuda", generator=g) for n in TG.NVEC], -1).float()
        ra, rc = torch.randn(N, 1, 128, device="cuda", generator=g), torch.randn(N, 1, 128, device="cuda", generator=g)
        adv, ret = torch.randn(T * N, 1, device="cuda", generator=g), torch.randn(T * N, 1, device="cuda", generator=g)
        for kind in ("reference", "fused"):
            pol = TG.Policy(seed=3)
            if kind == "fused":
                pkg.use_device_gru(pol)

            def step():
                values, logp, ent = pol.evaluate_actions(obs, ra, rc, act, m)
                ratio = torch.exp(logp - logp.detach())
                loss = -torch.min(ratio * adv, ratio.clamp(0.8, 1.2) * adv).mean() + 0.5 * (values - ret).pow(2).mean() - 0.01 * ent
                pol.optimizer.zero_grad()
                loss.backward()
            row(N, T, f"actor + critic minibatch, {kind} GRU", timed(step, max(5, a.reps // 2)))
        del x, h, m, go, obs, act
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
