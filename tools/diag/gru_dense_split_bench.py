#!/usr/bin/env python3
"""The fused GRU layer's split-bf16 dense products (dense_products="bf16x3") against its fp32 kernels on one MI355X ->
profiles/gru_dense_split_bench.txt ("The whole GRU layer").

For each (N chunks, T) shape, three consecutive runs, each the median of --reps calls per leg with the two legs
(dense_products="fp32", "bf16x3") alternating call by call on the same tensors (device = HIP events around each call, wall = per call
with a synchronise):

1. the forward C call (gi, recurrence, LayerNorm): the legs differ in gru_gi_fwd / gru_gi_fwd_b3 alone;
2. the backward C call without dx: the legs differ in gru_dw / gru_dw_b3 alone;
3. the backward C call with dx: leg 3 minus leg 2 is gru_dx / gru_dx_b3 alone;
   (1 - 3 with products="bf16x3", the shorter recurrence; the C entries have no call that launches one dense kernel by itself, the
   kernels' own times are in the rocprofv3 table at the end)
4. DeviceFusedGRULayer forward + backward, under products="bf16x3" and under products="fp32";
5. one actor + critic minibatch of the tests' restated policy through DevicePPOTrainer.ppo_update, under both products likewise;
6. with --parent-lib (a build of the parent commit): the untouched default (both selectors fp32, this tree's library) against the
   parent's ac_gru_layer_forward_p + ac_gru_layer_backward_p, the "fp32" column being the parent and the other this tree.

The verdict a split kernel is kept by: at 320 x 60 and at 4096 x 60 its time (legs 1, 2, 3 - 2, device) is below the fp32 kernel's
in each of the three runs by more than the largest run-to-run spread (max - min over the runs) of either leg at that shape.

Then, at 4096 x 60, rel = max|a - ref| / max|ref| against a float64 torch run of every output and gradient, for torch fp32 (the
reference's form), the fp32 kernels and the split kernels.

The kernels' own times come from a rocprofv3 kernel trace per shape, each a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/<N>x<T> -- python tools/diag/gru_dense_split_bench.py --trace <N>x<T>
    python tools/diag/gru_dense_split_bench.py --stats OUT
"""
import argparse
import csv
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gru_split_bench import DONE, H, ROOT, RUNS, SHAPES, VERDICT_SHAPES, U, Launch, pkg, timed_pair  # noqa: E402

FORMS = ("fp32", "bf16x3")
KERNELS = ("gru_gi_fwd", "gru_dw", "gru_dx")


def call_legs(N, T, parent=None, seed=0):
    """{what: (fp32 leg, bf16x3 leg)} of the C calls as closures over the same inputs; each form's backward reads what its own
    forward kept."""
    M = N * T
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.rand(*s, device="cuda", generator=g) * 2 - 1
    x, hxs, g_out, g_h = r(M, H) * 2, r(N, H), r(M, H), r(N, H)
    w_ih, w_hh, b_ih, b_hh = r(3 * H, H) / np.sqrt(H), r(3 * H, H) / np.sqrt(H), r(3 * H) / np.sqrt(H), r(3 * H) / np.sqrt(H)
    gamma, beta = 1 + 0.5 * r(H), 0.3 * r(H)
    masks = (torch.rand(M, device="cuda", generator=g) > DONE).float()
    run = Launch(x)
    new = run.empty

    def legs_of(fwd_call, bwd_call):
        gi, out, h_T, y, saved, stats = new(M * 3 * H), new(M, H), new(N, H), new(M, H), new(M, 4 * H), new(M, 2)
        ws = run.workspace("ac_gru_layer_workspace_floats", N, T)
        grads = [new(M, H), new(N, H), new(3 * H, H), new(3 * H, H), new(3 * H), new(3 * H), new(H), new(H)]
        fwd = lambda: fwd_call(N, T, x, hxs, masks, w_ih, w_hh, b_ih, b_hh, gamma, beta, 1e-5, gi, out, h_T, y, saved, stats)
        bwd = lambda dx: bwd_call(N, T, g_out, g_h, x, hxs, masks, w_ih, w_hh, gamma, y, saved, stats, ws, dx, *grads[1:])
        fwd()
        return fwd, (lambda: bwd(None)), (lambda: bwd(grads[0]))

    per = [legs_of(lambda *a, d=d: run("ac_gru_layer_forward_pd", *a, 1, d), lambda *a, d=d: run("ac_gru_layer_backward_pd", *a, 1, d)) for d in (0, 1)]
    legs = {"1. forward call (gi + recurrence + LayerNorm)": (per[0][0], per[1][0]),
            "2. backward call without dx (.. + dw)": (per[0][1], per[1][1]),
            "3. backward call with dx (.. + dw + dx)": (per[0][2], per[1][2])}
    if parent is not None:
        ptr = lambda a: a.data_ptr() if isinstance(a, torch.Tensor) else a

        def old(symbol):
            fn = getattr(parent, symbol)
            fn.restype, fn.argtypes = pkg.capi.SIGNATURES[symbol]

            def call(*a):
                if fn(run.dev.index, run.stream, *[ptr(v) for v in a], 0) != 0:
                    raise RuntimeError(symbol + " of the parent's library failed")
            return call
        pf, _, pb = legs_of(old("ac_gru_layer_forward_p"), old("ac_gru_layer_backward_p"))
        nf, _, nb = legs_of(lambda *a: run("ac_gru_layer_forward_pd", *a, 0, 0), lambda *a: run("ac_gru_layer_backward_pd", *a, 0, 0))
        legs["6. default, forward + backward calls: parent | this tree"] = ((lambda: (pf(), pb())), (lambda: (nf(), nb())))
    torch.cuda.synchronize()
    return legs


def layer_legs(N, T, products, seed=0):
    ref = U.RefGRULayer().cuda()
    layers = []
    for form in FORMS:
        h = torch.nn.Module()
        h.rnn = U.RefGRULayer().cuda()
        h.rnn.load_state_dict(ref.state_dict())
        assert pkg.use_device_gru_layer(h, products=products, dense_products=form) == 1 and h.rnn.dense_products == form
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


def minibatch_legs(N, T, products, seed=1):
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
        assert pkg.use_device_gru_layer(pol, products=products, dense_products=form) == 2 and pkg.use_device_mlp(pol) == 4 and pkg.use_device_act(pol) == 1
        legs.append(lambda pol=pol: trainer.ppo_update(pol, sample))
    return legs


def accuracy_lines(N=4096, T=60):
    """rel against float64 of every output and gradient: torch fp32, the fp32 kernels, the split kernels (products="fp32" throughout,
    so that the dense products alone differ)."""
    rel = lambda a, ref: float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))
    inp = U.random_inputs(N, T, done=DONE)

    def run(layer_fn, params, dt):
        c = lambda k, gr=False: torch.tensor(inp[k], dtype=dt, device="cuda", requires_grad=gr)
        for p in params.values():
            p.grad = None
        res = U.run_with_grads(layer_fn, params, c("x", True), c("hxs", True), c("masks"), c("g_out"), c("g_h"))
        torch.cuda.empty_cache()
        return res
    p64 = {k: torch.tensor(inp[k], dtype=torch.float64, device="cuda", requires_grad=True) for k in U.GRU_NAMES + U.NORM_NAMES}
    f64 = run(lambda x, h, m: U.step_layer(p64, x, h, m, N, T), p64, torch.float64)
    res = {}
    for tag, dense in (("torch fp32", None), ("fp32 kernels", "fp32"), ("split kernels", "bf16x3")):
        holder = torch.nn.Module()
        holder.rnn = U.layer_from(inp)
        if dense:
            assert pkg.use_device_gru_layer(holder, products="fp32", dense_products=dense) == 1
        res[tag] = run(holder.rnn, U.layer_params(holder.rnn), torch.float32)
    lines = [f"# errors at {N} x {T} (done rate {DONE}, products=\"fp32\"): rel = max|a - ref| / max|ref| against a float64 torch run; "
             "bound = max(4 x torch fp32, 2^-20)",
             f"{'key':8s} {'torch fp32':>11} {'fp32 kernels':>13} {'split kernels':>14} {'bound':>10} {'split / bound':>14}"]
    for k in U.KEYS:
        e = [rel(res[t][k], f64[k]) for t in ("torch fp32", "fp32 kernels", "split kernels")]
        b = max(4 * e[0], 2.0 ** -20)
        lines.append(f"{k:8s} {e[0]:11.2e} {e[1]:13.2e} {e[2]:14.2e} {b:10.2e} {e[2] / b:14.2f}")
    return lines


def trace(N, T, iters=10):
    legs = call_legs(N, T)
    for _ in range(iters):
        for fa, fb in list(legs.values())[::2]:   # the forward call and the backward call with dx, both forms
            fa(); fb()
    torch.cuda.synchronize()


def stats_lines(stats_dir):
    lines = ["# rocprofv3 --kernel-trace --stats of the six dense kernels, a run per shape (us per launch)",
             f"{'N':>6} {'T':>3} {'kernel':18s} {'calls':>6} {'avg':>9} {'min':>9} {'max':>9}"]
    found = False
    shape_of = lambda d: tuple(int(v) for v in os.path.basename(d).split("x"))
    for d in sorted(glob.glob(os.path.join(stats_dir, "*x*")), key=lambda d: SHAPES.index(shape_of(d)) if shape_of(d) in SHAPES else len(SHAPES)) if stats_dir else []:
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            continue
        N, T = shape_of(d)
        rows = {}
        for row in csv.DictReader(open(files[0])):
            rows[row["Name"].replace("void ", "").split("(")[0].split("::")[-1]] = row
        for name in (k + s for k in KERNELS for s in ("", "_b3")):
            if name in rows:
                found, row = True, rows[name]
                lines.append(f"{N:6d} {T:3d} {name:18s} {int(row['Calls']):6d} {float(row['AverageNs']) / 1e3:9.1f} {float(row['MinNs']) / 1e3:9.1f} "
                             f"{float(row['MaxNs']) / 1e3:9.1f}")
    return lines if found else lines[:1] + ["  no trace given"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_dense_split_bench.txt"))
    ap.add_argument("--shapes", default="")
    ap.add_argument("--parent-lib", default="", help="libaircombat_hip.so built from the parent commit, for leg 6")
    ap.add_argument("--no-errors", action="store_true", help="skip the error table at 4096 x 60")
    ap.add_argument("--trace", default="", help="NxT: the C calls in both forms at that shape, for a rocprofv3 kernel trace")
    ap.add_argument("--stats", default=None, help="directory of the kernel traces: <stats>/<N>x<T>/**/*kernel_stats.csv")
    a = ap.parse_args()
    if a.trace:
        return trace(*(int(v) for v in a.trace.split("x")))
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")] if a.shapes else SHAPES
    parent = ctypes.CDLL(a.parent_lib) if a.parent_lib else None
    lines = [f"# tools/diag/gru_dense_split_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, done rate {DONE}; {RUNS} consecutive "
             f"runs, each the median of {a.reps} calls per leg (ms), the legs alternating call by call: device = HIP events around each call, "
             "wall = per call with a synchronise"]
    try:
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        rev = ""
    lines.append(f"# {'parent commit ' + rev + ' plus ' if rev else ''}the working tree of this change; fp32 = the parent's kernels, unchanged; legs 1 - 3 "
                 "with products=\"bf16x3\"")
    lines.append(f"{'N':>6} {'T':>3} {'what':58s} {'run':>3} {'fp32 dev':>9} {'bf16x3 dev':>10} {'fp32 wall':>9} {'bf16x3 wall':>11}")
    slower, dev = [], {}
    for N, T in shapes:
        calls = call_legs(N, T, parent)
        todo = [(what, lambda pair=pair: pair) for what, pair in calls.items() if what[0] != "6"]
        for products in FORMS[::-1]:
            todo.append((f"4. fused layer, forward + backward, products={products}", lambda p=products: layer_legs(N, T, p)))
        for products in FORMS[::-1]:
            todo.append((f"5. actor + critic minibatch, DevicePPOTrainer, products={products}", lambda p=products: minibatch_legs(N, T, p)))
        todo += [(what, lambda pair=pair: pair) for what, pair in calls.items() if what[0] == "6"]
        for what, legs in todo:
            fa, fb = legs()
            for run in range(RUNS):
                (pd, pw), (nd, nw) = timed_pair(fa, fb, a.reps)
                lines.append(f"{N:6d} {T:3d} {what:58s} {run + 1:3d} {pd:9.3f} {nd:10.3f} {pw:9.3f} {nw:11.3f}")
                print(lines[-1], flush=True)
                if nd > pd or nw > pw:
                    slower.append((N, T, what, run + 1))
                if what[0] in "123":
                    dev.setdefault((N, T), {}).setdefault(what[0], []).append((pd, nd))
            del fa, fb
            torch.cuda.empty_cache()
        del calls, todo
        torch.cuda.empty_cache()
    lines.append("# second column slower than the first (device or wall): " + (", ".join(f"{n} x {t} leg {w[:2]}{' ' + w.split()[-1] if 'products=' in w else ''} run {r}" for n, t, w, r in slower) or "nowhere"))
    kept = {k: True for k in KERNELS}
    for shape in VERDICT_SHAPES:
        if shape not in dev:
            continue
        d = {k: np.array(v) for k, v in dev[shape].items()}
        for kernel, s in zip(KERNELS, (d["1"], d["2"], d["3"] - d["2"])):
            spread = float(max(np.ptp(s[:, 0]), np.ptp(s[:, 1])))
            ok = bool((s[:, 0] - s[:, 1] > spread).all())
            kept[kernel] &= ok
            how = {"gru_gi_fwd": "leg 1", "gru_dw": "leg 2", "gru_dx": "leg 3 - leg 2"}[kernel]
            lines.append(f"# verdict {shape[0]} x {shape[1]} {kernel}_b3 ({how}), device ms per run: fp32 {', '.join(f'{v:.3f}' for v in s[:, 0])}; "
                         f"bf16x3 {', '.join(f'{v:.3f}' for v in s[:, 1])}; largest run-to-run spread {spread:.3f}; "
                         f"bf16x3 faster by more than that in every run: {'yes' if ok else 'NO'}")
    for kernel in KERNELS:
        lines.append(f"# condition for keeping {kernel}_b3: {'met' if kept[kernel] else 'NOT met'}")
    if not a.no_errors:
        lines += accuracy_lines()
    lines += stats_lines(a.stats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-40:]))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
