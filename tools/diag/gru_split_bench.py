#!/usr/bin/env python3
"""The training GRU's split-bf16 product against the exact-fp32 one on one MI355X -> profiles/gru_split_bench.txt ("The
training GRU").

For each (N chunks, T) shape, three consecutive runs, each the median of --reps calls per leg with the two legs (products="fp32",
products="bf16x3") alternating call by call on the same tensors (device = HIP events around each call, wall = per call with a
synchronise):

1. the recurrence forward alone (ac_gru_seq_forward_p, with ``saved``);
2. the recurrence backward alone (ac_gru_seq_backward_p, with ``dhxs``);
3. DeviceFusedGRULayer, forward + backward;
4. one actor + critic minibatch of the tests' restated policy through DevicePPOTrainer.ppo_update with every layer swapped.

The verdict the change is kept by: at 320 x 60 and at 4096 x 60 the recurrence forward + backward (legs 1 + 2, device time) with bf16x3
is below fp32's in each of the three runs by more than the largest run-to-run spread (max - min over the runs) of either leg's sum at
that shape.

The kernels' own times come from a rocprofv3 kernel trace per shape, each a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/<N>x<T> -- python tools/diag/gru_split_bench.py --trace <N>x<T>
    python tools/diag/gru_split_bench.py --stats OUT
"""
import argparse
import csv
import glob
import importlib
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
Launch = importlib.import_module("aircombat-selfplay_amd.train_common").Launch

SHAPES = [(320, 60), (2400, 8), (4096, 60), (16384, 8)]
VERDICT_SHAPES = [(320, 60), (4096, 60)]
DONE = 0.02
RUNS = 3
H = 128
FORMS = ("fp32", "bf16x3")


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


def recurrence_legs(N, T, seed=0):
    """((forward fp32, forward bf16x3), (backward fp32, backward bf16x3)) as closures over the same tensors; each form's backward reads
    what its own forward saved."""
    M = N * T
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.rand(*s, device="cuda", generator=g) * 2 - 1
    gi, hxs, w_hh, b_hh = r(M, 3 * H) * 2, r(N, H), r(3 * H, H) / np.sqrt(H), r(3 * H) / np.sqrt(H)
    masks = (torch.rand(M, device="cuda", generator=g) > DONE).float()
    dy, dh_T = r(M, H), r(N, H)
    run = Launch(gi)
    fwd, bwd = [], []
    for code in (0, 1):
        y, h_T, saved = run.empty(M, H), run.empty(N, H), run.empty(M, 4 * H)
        dgi, dgh, dhxs = run.empty(M, 3 * H), run.empty(M, 3 * H), run.empty(N, H)
        f = lambda y=y, h_T=h_T, saved=saved, code=code: run("ac_gru_seq_forward_p", N, T, gi, hxs, masks, w_hh, b_hh, y, h_T, saved, code)
        f()
        fwd.append(f)
        bwd.append(lambda y=y, saved=saved, dgi=dgi, dgh=dgh, dhxs=dhxs, code=code:
                   run("ac_gru_seq_backward_p", N, T, dy, dh_T, saved, y, hxs, masks, w_hh, dgi, dgh, dhxs, code))
    torch.cuda.synchronize()
    return fwd, bwd


def layer_legs(N, T, seed=0):
    ref = U.RefGRULayer().cuda()
    layers = []
    for form in FORMS:
        h = torch.nn.Module()
        h.rnn = U.RefGRULayer().cuda()
        h.rnn.load_state_dict(ref.state_dict())
        assert pkg.use_device_gru_layer(h, products=form) == 1 and h.rnn.products == form
        layers.append(h.rnn)
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(T * N, H, device="cuda", generator=g, requires_grad=True)
    h0 = torch.randn(N, 1, H, device="cuda", generator=g, requires_grad=True)
    m = (torch.rand(T * N, 1, device="cuda", generator=g) > DONE).float()
    go = torch.randn(T * N, H, device="cuda", generator=g)

    def fwdbwd(layer):
        out, _ = layer(x, h0, m)
        (out * go).sum().backward()
    return [lambda layer=layer: fwdbwd(layer) for layer in layers]


def minibatch_legs(N, T, seed=1):
    M = N * T
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    act = torch.stack([torch.randint(0, n, (M,), device="cuda", generator=g) for n in U.NVEC], -1).float()
    masks = (torch.rand(M, 1, device="cuda", generator=g) > DONE).float()
    sample = (r(M, U.OBS), act, masks, r(M, 1) * 0.1 - 2.0, r(M, 1), r(M, 1), r(M, 1), r(N, 1, H), r(N, 1, H))
    trainer = pkg.DevicePPOTrainer(U.trainer_args(), torch.device("cuda", 0))
    legs = []
    for form in FORMS:
        pol = U.Policy(seed=3)
        assert pkg.use_device_gru_layer(pol, products=form) == 2 and pkg.use_device_mlp(pol) == 4 and pkg.use_device_act(pol) == 1
        legs.append(lambda pol=pol: trainer.ppo_update(pol, sample))
    return legs


def trace(N, T, iters=10):
    fwd, bwd = recurrence_legs(N, T)
    for _ in range(iters):
        for f in fwd + bwd:
            f()
    torch.cuda.synchronize()


def stats_lines(stats_dir):
    lines = ["# rocprofv3 --kernel-trace --stats of the four recurrence kernels alone, a run per shape (us per launch)",
             f"{'N':>6} {'T':>3} {'kernel':18s} {'calls':>6} {'avg':>9} {'min':>9} {'max':>9}"]
    found = False
    for d in sorted(glob.glob(os.path.join(stats_dir, "*x*"))) if stats_dir else []:
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            continue
        N, T = (int(v) for v in os.path.basename(d).split("x"))
        for row in csv.DictReader(open(files[0])):
            name = row["Name"].replace("void ", "").split("(")[0].split("::")[-1]
            if name.startswith("gru_seq_"):
                found = True
                lines.append(f"{N:6d} {T:3d} {name:18s} {int(row['Calls']):6d} {float(row['AverageNs']) / 1e3:9.1f} {float(row['MinNs']) / 1e3:9.1f} "
                             f"{float(row['MaxNs']) / 1e3:9.1f}")
    return lines if found else lines[:1] + ["  no trace given"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_split_bench.txt"))
    ap.add_argument("--shapes", default="")
    ap.add_argument("--trace", default="", help="NxT: the four recurrence kernels alone at that shape, for a rocprofv3 kernel trace")
    ap.add_argument("--stats", default=None, help="directory of the kernel traces: <stats>/<N>x<T>/**/*kernel_stats.csv")
    a = ap.parse_args()
    if a.trace:
        return trace(*(int(v) for v in a.trace.split("x")))
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")] if a.shapes else SHAPES
    lines = [f"# tools/diag/gru_split_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, done rate {DONE}; {RUNS} consecutive runs, "
             f"each the median of {a.reps} calls per leg (ms), the legs alternating call by call: device = HIP events around each call, "
             "wall = per call with a synchronise"]
    try:
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        rev = ""
    lines.append(f"# {'parent commit ' + rev + ' plus ' if rev else ''}the working tree of this change; fp32 = the parent's kernels, unchanged")
    lines.append(f"{'N':>6} {'T':>3} {'what':46s} {'run':>3} {'fp32 dev':>9} {'bf16x3 dev':>10} {'fp32 wall':>9} {'bf16x3 wall':>11}")
    slower, sums = [], {}
    for N, T in shapes:
        fwd, bwd = recurrence_legs(N, T)
        for what, legs in (("1. recurrence forward", lambda: fwd), ("2. recurrence backward", lambda: bwd),
                           ("3. fused layer, forward + backward", lambda: layer_legs(N, T)),
                           ("4. actor + critic minibatch, DevicePPOTrainer", lambda: minibatch_legs(N, T))):
            fa, fb = legs()
            for run in range(RUNS):
                (pd, pw), (nd, nw) = timed_pair(fa, fb, a.reps)
                lines.append(f"{N:6d} {T:3d} {what:46s} {run + 1:3d} {pd:9.3f} {nd:10.3f} {pw:9.3f} {nw:11.3f}")
                print(lines[-1], flush=True)
                if nd > pd or nw > pw:
                    slower.append((N, T, what, run + 1))
                if what[0] in "12":
                    s = sums.setdefault((N, T), [[0.0, 0.0] for _ in range(RUNS)])
                    s[run][0] += pd
                    s[run][1] += nd
            del fa, fb
            torch.cuda.empty_cache()
        del fwd, bwd
    lines.append("# bf16x3 slower than fp32 (device or wall): " + (", ".join(f"{n} x {t} {w[:2]} run {r}" for n, t, w, r in slower) or "nowhere"))
    kept = True
    for shape in VERDICT_SHAPES:
        if shape not in sums:
            continue
        s = np.array(sums[shape])
        spread = float(max(np.ptp(s[:, 0]), np.ptp(s[:, 1])))
        gain = s[:, 0] - s[:, 1]
        ok = bool((gain > spread).all())
        kept &= ok
        lines.append(f"# verdict {shape[0]} x {shape[1]}: recurrence forward + backward, device ms per run: fp32 {', '.join(f'{v:.3f}' for v in s[:, 0])}; "
                     f"bf16x3 {', '.join(f'{v:.3f}' for v in s[:, 1])}; largest run-to-run spread {spread:.3f}; "
                     f"bf16x3 faster by more than that in every run: {'yes' if ok else 'NO'}")
    lines.append(f"# condition for keeping the split kernels: {'met' if kept else 'NOT met'}")
    lines += stats_lines(a.stats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-24:]))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
