#!/usr/bin/env python3
"""The whole GRU layer on one MI355X -> profiles/gru_layer_bench.txt ("The whole GRU layer").

For each (N chunks, T) shape, three consecutive runs, each the median of --reps calls per leg with the two legs alternating call by
call (device = HIP events around each call, wall = per call with a synchronise):

1. the layer alone, forward + backward: DeviceGRULayer (the recurrence on the device, the dense products and the LayerNorm torch)
   against DeviceFusedGRULayer (everything csrc/gru_layer_train.hpp);
2. one actor + critic minibatch of the tests' restated policy through DevicePPOTrainer.ppo_update after use_device_gru +
   use_device_mlp + use_device_act, without and with use_device_gru_layer.

3. The kernels' own times come from a rocprofv3 kernel trace of the layer at 4096 x 60, one leg per run, each a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/<leg> -- python tools/diag/gru_layer_bench.py --trace --leg <parent|new>
    python tools/diag/gru_layer_bench.py --stats OUT

   The new kernels are listed with the bytes they must move (computed from the shape: every array read or written once, the weights
   left out) and that over their time as a share of the 8.0 TB/s HBM peak; for the parent leg, the kernels it launches and the new leg
   does not.
"""
import argparse
import csv
import glob
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
import gru_layer_util as U  # noqa: E402  (the tests' restatement of the reference's GRULayer, actor, critic and policy)

SHAPES = [(320, 60), (2400, 8), (4096, 60), (16384, 8)]
TRACE_SHAPE = (4096, 60)
DONE = 0.02
HBM_PEAK = 8.0e12
RUNS = 3


def kernel_bytes(N, T):
    """Bytes each new kernel must move at (N, T): name -> bytes."""
    M = N * T
    lib = pkg.load_library()
    tiles = -(-M // lib.ac_gru_layer_constant(0))
    dw_sets, ln_sets = 2 * min(tiles, lib.ac_gru_layer_constant(4)), min(tiles, lib.ac_gru_layer_constant(3))
    part = 4 * (dw_sets * (384 * 128 + 384) + ln_sets * 256)
    return {"gru_gi_fwd": M * 4 * (128 + 384), "gru_ln_fwd": M * 4 * (128 + 128 + 2), "gru_ln_bwd": M * 4 * (128 + 128 + 2 + 128),
            "gru_dw": M * 4 * (384 + 384 + 128 + 128 + 1) + 4 * dw_sets * (384 * 128 + 384), "gru_dx": M * 4 * (384 + 128),
            "gru_sum_partials": part, "gru_seq_fwd": M * 4 * (384 + 128 + 512 + 1), "gru_seq_bwd": M * 4 * (128 + 512 + 128 + 1 + 384 + 384)}


def timed_pair(fa, fb, reps, warm=3):
    """Medians (device ms, wall ms) of fa and of fb, the two alternating call by call."""
    for _ in range(warm):
        fa(); fb()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e0, e1, e2 in ev:
        e0.record(); fa(); e1.record(); fb(); e2.record()
    torch.cuda.synchronize()
    dev = [float(np.median([e[i].elapsed_time(e[i + 1]) for e in ev])) for i in (0, 1)]
    wall = ([], [])
    for _ in range(reps):
        for i, fn in enumerate((fa, fb)):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); wall[i].append((time.perf_counter() - t0) * 1e3)
    return (dev[0], float(np.median(wall[0]))), (dev[1], float(np.median(wall[1])))


def layer_legs(N, T, seed=0):
    """(parent layer, new layer, forward + backward of a layer) on the same seeded inputs and parameters."""
    ref = U.RefGRULayer().cuda()
    holders = []
    for swap in (pkg.use_device_gru, pkg.use_device_gru_layer):
        h = torch.nn.Module()
        h.rnn = U.RefGRULayer().cuda()
        h.rnn.load_state_dict(ref.state_dict())
        assert swap(h) == 1
        holders.append(h.rnn)
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(T * N, 128, device="cuda", generator=g, requires_grad=True)
    h0 = torch.randn(N, 1, 128, device="cuda", generator=g, requires_grad=True)
    m = (torch.rand(T * N, 1, device="cuda", generator=g) > DONE).float()
    go = torch.randn(T * N, 128, device="cuda", generator=g)

    def fwdbwd(layer):
        out, _ = layer(x, h0, m)
        (out * go).sum().backward()
    return holders[0], holders[1], fwdbwd


def minibatch_legs(N, T, seed=1):
    """The two whole-minibatch legs: DevicePPOTrainer.ppo_update on the tests' policy with the three swaps, and with the fourth."""
    M = N * T
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    act = torch.stack([torch.randint(0, n, (M,), device="cuda", generator=g) for n in U.NVEC], -1).float()
    masks = (torch.rand(M, 1, device="cuda", generator=g) > DONE).float()
    sample = (r(M, U.OBS), act, masks, r(M, 1) * 0.1 - 2.0, r(M, 1), r(M, 1), r(M, 1), r(N, 1, 128), r(N, 1, 128))
    trainer = pkg.DevicePPOTrainer(U.trainer_args(), torch.device("cuda", 0))
    legs = []
    for fused in (False, True):
        pol = U.Policy(seed=3)
        assert pkg.use_device_gru(pol) == 2 and pkg.use_device_mlp(pol) == 4 and pkg.use_device_act(pol) == 1
        if fused:
            assert pkg.use_device_gru_layer(pol) == 2
        legs.append(lambda pol=pol: trainer.ppo_update(pol, sample))
    return legs


def read_stats(stats_dir, leg):
    files = glob.glob(os.path.join(stats_dir, leg, "**", "*kernel_stats.csv"), recursive=True)
    return {r["Name"]: (int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(open(files[0]))} if files else None


def trace_lines(stats_dir):
    N, T = TRACE_SHAPE
    lines = [f"# 3. rocprofv3 --kernel-trace --stats of the layer alone, forward + backward, at {N} x {T}, one leg per run"]
    legs = {leg: read_stats(stats_dir, leg) for leg in ("parent", "new")} if stats_dir else {"parent": None, "new": None}
    if legs["parent"] is None or legs["new"] is None:
        return lines + ["  no trace given"]
    short = lambda n: n.replace("void ", "").replace("(anonymous namespace)::", "").replace("at::native::", "").split("(")[0][:70]
    nbytes = kernel_bytes(N, T)
    lines.append(f"  new leg: {'kernel':40s} {'calls':>6} {'us/call':>9} {'MB':>8} {'%HBM':>6}")
    for name, (calls, avg) in sorted(legs["new"].items(), key=lambda kv: -kv[1][0] * kv[1][1]):
        key = next((k for k in nbytes if k in name), None)
        if key is None:
            lines.append(f"           {short(name):40s} {calls:6d} {avg / 1e3:9.1f}   (not one of the layer's kernels)")
            continue
        lines.append(f"           {key:40s} {calls:6d} {avg / 1e3:9.1f} {nbytes[key] / 1e6:8.1f} {100 * nbytes[key] / (avg * 1e-9) / HBM_PEAK:6.1f}")
    lines.append("  parent leg, the kernels it launches and the new leg does not:")
    for name, (calls, avg) in sorted(legs["parent"].items(), key=lambda kv: -kv[1][0] * kv[1][1]):
        if name not in legs["new"]:
            lines.append(f"           {short(name):70s} {calls:6d} {avg / 1e3:9.1f}")
    for leg in ("parent", "new"):
        its = min(c for n, (c, _) in legs[leg].items() if "gru_seq_fwd" in n)
        lines.append(f"  {leg} leg: kernel time per forward + backward {sum(c * a for c, a in legs[leg].values()) / its / 1e3:9.1f} us ({its} iterations)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_layer_bench.txt"))
    ap.add_argument("--shapes", default="")
    ap.add_argument("--trace", action="store_true", help="the layer alone at 4096 x 60, one leg, for a rocprofv3 kernel trace")
    ap.add_argument("--leg", default="new", choices=["parent", "new"])
    ap.add_argument("--stats", default=None, help="directory of the kernel traces: <stats>/<leg>/**/*kernel_stats.csv")
    a = ap.parse_args()
    if a.trace:
        parent, new, fwdbwd = layer_legs(*TRACE_SHAPE)
        layer = parent if a.leg == "parent" else new
        for _ in range(10):
            fwdbwd(layer)
        torch.cuda.synchronize()
        return
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")] if a.shapes else SHAPES
    lines = [f"# tools/diag/gru_layer_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, done rate {DONE}; {RUNS} consecutive runs, "
             f"each the median of {a.reps} calls per leg (ms), the legs alternating call by call: device = HIP events around each call, "
             "wall = per call with a synchronise"]
    try:
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        lines.append(f"# parent commit {rev or '?'} plus the working tree of this change")
    except OSError:
        pass
    lines.append(f"{'N':>6} {'T':>3} {'what':46s} {'run':>3} {'parent dev':>10} {'new dev':>9} {'parent wall':>11} {'new wall':>9}")
    slower = []
    for N, T in shapes:
        for what, make in (("1. layer alone, forward + backward", None), ("2. actor + critic minibatch, DevicePPOTrainer", minibatch_legs)):
            if make is None:
                parent, new, fwdbwd = layer_legs(N, T)
                fa, fb = (lambda: fwdbwd(parent)), (lambda: fwdbwd(new))
            else:
                fa, fb = make(N, T)
            for run in range(RUNS):
                (pd, pw), (nd, nw) = timed_pair(fa, fb, a.reps)
                lines.append(f"{N:6d} {T:3d} {what:46s} {run + 1:3d} {pd:10.3f} {nd:9.3f} {pw:11.3f} {nw:9.3f}")
                print(lines[-1], flush=True)
                if nd > pd or nw > pw:
                    slower.append((N, T, what, run + 1))
            del fa, fb
            torch.cuda.empty_cache()
    lines.append("# new leg slower than the parent leg (device or wall): " + (", ".join(f"{n} x {t} {w[:2]} run {r}" for n, t, w, r in slower) or "nowhere"))
    lines += trace_lines(a.stats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-40:]))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
