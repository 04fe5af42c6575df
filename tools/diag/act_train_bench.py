#!/usr/bin/env python3
"""Training action-head timings on one MI355X -> profiles/act_train_bench.txt ("The training action heads").

For each (N chunks, T) shape, M = N * T rows, and each action space ([3, 5, 3]; [3, 5, 3] + [2, 2, 2, 2] with the shoot priors and
active_masks; [41, 41, 41, 30]): the heads alone, evaluate_actions under no_grad and evaluate_actions + backward of a loss on both
outputs, fused (use_device_act) against the very same modules in eager torch (the tests' restatement of the reference's ACTLayer, a
torch.distributions object per head). Then one whole actor + critic evaluate_actions + PPO loss + loss.backward() minibatch for the
last two spaces with (a) use_device_gru + use_device_mlp, the state before the fused heads existed, and (b) use_device_act as well. The
members of each comparison alternate call by call within the run. Each is reported as the median HIP-event time over the calls and the
median wall time per call with a synchronise, after warm-up. The fused heads-alone rows also carry the bytes the heads have to move
(from the shape: x, the actions, the priors, logp and ent, and in the backward their gradients and dx; the parameters and the partial
sums are left out) and that over the device time as a share of the 8.0 TB/s HBM peak.

    python tools/diag/act_train_bench.py [--reps 20] [--out profiles/act_train_bench.txt] [--shapes 4096x60,320x60]
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
import act_train_util as U  # noqa: E402  (the tests' restatement of the reference's ACTLayer and actor, whose heads are modules that are called)
import mlp_train_util as MU  # noqa: E402

SHAPES = [(320, 60), (2400, 8), (4096, 60), (16384, 8)]
SPACES = [((3, 5, 3), 0), ((3, 5, 3), 4), ((41, 41, 41, 30), 0)]
DONE = 0.02
HBM_PEAK = 8.0e12


def space_name(nvec, ns):
    return str(list(nvec)) + (f" + {[2] * ns}" if ns else "")


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


def inputs(M, nvec, ns, g):
    sizes = list(nvec) + [2] * ns
    act = torch.stack([torch.randint(0, n, (M,), device="cuda", generator=g) for n in sizes], -1).float()
    kw = {}
    if ns:
        pick = lambda vals: torch.tensor(vals, device="cuda")[torch.randint(0, 3, (M, 1), device="cuda", generator=g)]
        kw = {"alpha0": pick(U.ALPHA0), "beta0": pick(U.BETA0)}
    active = (torch.rand(M, 1, device="cuda", generator=g) > 0.1).float() if ns else None
    return act, active, kw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "act_train_bench.txt"))
    ap.add_argument("--shapes", default="")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")] if a.shapes else SHAPES
    torch.manual_seed(0)
    lines = [f"# tools/diag/act_train_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, median of {a.reps} (ms): "
             f"device = HIP events over back-to-back calls, wall = per call with a synchronise; MB = what the fused heads must move, "
             f"%HBM = MB / device time over {HBM_PEAK / 1e12:.1f} TB/s"]
    try:
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        lines.append(f"# parent commit {rev or '?'} plus the working tree of this change")
    except OSError:
        pass
    lines.append(f"{'N':>6} {'T':>3} {'what':76s} {'device':>9} {'wall':>9} {'MB':>8} {'%HBM':>6}")

    def row(N, T, what, r, nbytes=None):
        tail = f" {nbytes / 1e6:8.1f} {100 * nbytes / (r[0] * 1e-3) / HBM_PEAK:6.1f}" if nbytes else ""
        lines.append(f"{N:6d} {T:3d} {what:76s} {r[0]:9.3f} {r[1]:9.3f}{tail}")
        print(lines[-1], flush=True)

    for N, T in shapes:
        M = N * T
        g = torch.Generator(device="cuda").manual_seed(0)
        for nvec, ns in SPACES:
            eager = U.Act(nvec, ns).cuda()
            fused = copy.deepcopy(eager)
            assert pkg.use_device_act(fused) == 1
            x = torch.randn(M, 128, device="cuda", generator=g, requires_grad=True)
            act, active, kw = inputs(M, nvec, ns, g)
            g1, g2 = torch.randn(M, 1, device="cuda", generator=g), torch.randn(M, 1, device="cuda", generator=g)
            name = space_name(nvec, ns)

            def fwd(m):
                with torch.no_grad():
                    m.evaluate_actions(x, act, active, **kw)

            def fwdbwd(m):
                logp, ent = m.evaluate_actions(x, act, active, **kw)
                wrt = [x] + [p for i in U.used_heads((M, nvec, ns, False)) for p in m.action_outs[i].parameters()]
                torch.autograd.grad((logp * g1).sum() + (ent * g2).sum(), wrt)

            cols = len(nvec) + ns + (2 if ns else 0)   # action columns and the two priors
            r = timed([lambda: fwd(fused), lambda: fwd(eager)], a.reps)
            row(N, T, f"heads {name}: fused evaluate_actions (no_grad)", r[0], 4 * M * (128 + cols + 2))
            row(N, T, f"heads {name}: eager evaluate_actions (no_grad)", r[1])
            r = timed([lambda: fwdbwd(fused), lambda: fwdbwd(eager)], a.reps)
            # forward: x, actions, priors, logp, ent; backward: the same inputs, dlogp, dent and dx
            row(N, T, f"heads {name}: fused evaluate_actions + backward", r[0], 4 * M * ((128 + cols + 2) + (128 + cols + 2) + 128))
            row(N, T, f"heads {name}: eager evaluate_actions + backward", r[1])
            del x, act, g1, g2
        # one whole actor + critic minibatch: evaluate_actions + PPO loss + backward
        for nvec, ns in SPACES[1:]:
            g = torch.Generator(device="cuda").manual_seed(1)
            obs = torch.randn(M, MU.OBS, device="cuda", generator=g)
            act, active, kw = inputs(M, nvec, ns, g)
            ra, rc = torch.randn(N, 1, 128, device="cuda", generator=g), torch.randn(N, 1, 128, device="cuda", generator=g)
            adv, ret = torch.randn(M, 1, device="cuda", generator=g), torch.randn(M, 1, device="cuda", generator=g)
            m = (torch.rand(M, 1, device="cuda", generator=g) > DONE).float()
            pol_parent = U.Policy(seed=3, nvec=nvec, ns=ns)
            assert pkg.use_device_gru(pol_parent) == 2 and pkg.use_device_mlp(pol_parent) == 4
            pol_act = copy.deepcopy(pol_parent)
            assert pkg.use_device_act(pol_act) == 1

            def step(pol):
                logp, ent = pol.actor.evaluate_actions(obs, ra, act, m, active, **kw)
                values, _ = pol.critic(obs, rc, m)
                ratio = torch.exp(logp - logp.detach())
                loss = -torch.min(ratio * adv, ratio.clamp(0.8, 1.2) * adv).mean() + 0.5 * (values - ret).pow(2).mean() - 0.01 * ent.sum()
                pol.optimizer.zero_grad()
                loss.backward()

            r = timed([lambda: step(pol_parent), lambda: step(pol_act)], max(5, a.reps // 2))
            row(N, T, f"actor + critic minibatch {space_name(nvec, ns)}, fused GRU + MLP", r[0])
            row(N, T, f"actor + critic minibatch {space_name(nvec, ns)}, fused GRU + MLP + heads", r[1])
            del obs, act, m, adv, ret
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
