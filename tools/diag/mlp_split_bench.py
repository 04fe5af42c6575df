#!/usr/bin/env python3
"""The training MLP blocks' split-bf16 products (products="bf16x3") against their fp32 kernels on one MI355X ->
profiles/mlp_split_bench.txt ("The training MLP blocks").

For each (N chunks, T) shape, M = N T rows, three consecutive runs, each the median of --reps calls per leg with the two legs
(products="fp32", "bf16x3") alternating call by call on the same tensors (device = HIP events around each call, wall = per call with a
synchronise):

a. the kernels one by one, per K in 15, 32, 64, 128 (the fp32 form pads K = 15 to 16): the forward call in its inference form (no
   statistics kept), the backward call with dx and the backward call without dx (each backward call is the block's kernel plus the
   same small sum of the partials in both forms). Only KP = 128 has split kernels (mlps::KPS), so at K <= 64 both legs run the fp32
   kernels and tie. Part 1 of profiles/mlp_split_bench.txt, measured with KP = 32, 64 and 128 dispatched, cannot be reproduced from
   this tree: the KP = 32 and 64 instantiations were removed after it, and measuring another dispatch mask needs the commit that
   added the split blocks, built with KPS = 32 | 64 | 128;
b. the forward + backward calls with dx at K = 128 and without dx at K = 15 (a head's block and an observation's);
c. a two-block DeviceMLPLayer, forward + backward: 128 -> 128 -> 128 with a gradient for x and 15 -> 128 -> 128 without;
d. one actor + critic minibatch of the tests' restated policy through DevicePPOTrainer.ppo_update, the fused GRU layer in its bf16x3
   forms (products and dense_products) and the action heads on the device, the MLP blocks in either form;
e. with --parent-lib (a build of the parent commit): the untouched default (ac_mlp_block_forward + ac_mlp_block_backward of this
   tree's library, K = 128 with dx) against the same calls of the parent's, the "fp32" column being the parent and the other this tree.

The verdict a split kernel is kept by (forward, backward with dx, backward without dx, per KP): at 4096 x 60 and at 16384 x 8 its
device time (legs a) is below the fp32 kernel's in each of the three runs by more than the largest run-to-run spread (max - min over
the runs) of either leg at that shape.

Then, at 4096 x 60, rel = max|a - ref| / max|ref| against a float64 torch run of every result of a two-block layer, for torch fp32,
the fp32 kernels and the split kernels. The ReLU is discontinuous in the backward, so the upstream gradient is zeroed on every row
that has a float64 pre-activation of either block below 2^-14 in magnitude (tests/test_gpu_mlp_split.py); the table says how many.

The kernels' own times come from a rocprofv3 kernel trace per shape, each a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/<N>x<T> -- python tools/diag/mlp_split_bench.py --trace <N>x<T>
    python tools/diag/mlp_split_bench.py --stats OUT
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
from gru_split_bench import DONE, H, ROOT, RUNS, SHAPES, U, Launch, pkg, timed_pair  # noqa: E402
import mlp_split_util as S  # noqa: E402  (tests/: the inputs of the errors table)
import mlp_train_util as MU  # noqa: E402

FORMS = ("fp32", "bf16x3")
VERDICT_SHAPES = [(4096, 60), (16384, 8)]
KS = (15, 32, 64, 128)
KINDS = ("forward", "backward with dx", "backward without dx")


def block_calls(M, K, seed=0, lib=None):
    """[(forward without statistics, forward with, backward with dx, backward without dx) per form] as closures over the same inputs;
    each form's backward reads what its own forward kept. ``lib``: the calls without ``products`` once, of that library (a ctypes
    handle) or, "tree", of this tree's."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    x, dy = r(M, K), r(M, H)
    w, b, gamma, beta = r(H, K) / np.sqrt(K), 0.1 * r(H), 1 + 0.3 * r(H), 0.3 * r(H)
    run = Launch(x)
    new = run.empty
    ptr = lambda a: a.data_ptr() if isinstance(a, torch.Tensor) else a

    def calls_of(fwd_call, bwd_call):
        y, stats, ws = new(M, H), new(M, 2), run.workspace("ac_mlp_block_workspace_floats", M, K)
        dx, grads = new(M, K), [new(H, K), new(H), new(H), new(H)]
        fwd = lambda st: fwd_call(M, K, 1e-5, x, w, b, gamma, beta, y, st)
        bwd = lambda d: bwd_call(M, K, dy, x, w, b, gamma, stats, ws, d, *grads)
        fwd(stats)
        return (lambda: fwd(None)), (lambda: fwd(stats)), (lambda: bwd(dx)), (lambda: bwd(None))

    if lib == "tree":
        return [calls_of(lambda *a: run("ac_mlp_block_forward", *a), lambda *a: run("ac_mlp_block_backward", *a))]
    if lib is not None:
        def old(symbol):
            fn = getattr(lib, symbol)
            fn.restype, fn.argtypes = pkg.capi.SIGNATURES[symbol]

            def call(*a):
                if fn(run.dev.index, run.stream, *[ptr(v) for v in a]) != 0:
                    raise RuntimeError(symbol + " failed")
            return call
        return [calls_of(old("ac_mlp_block_forward"), old("ac_mlp_block_backward"))]
    out = [calls_of(lambda *a, c=c: run("ac_mlp_block_forward_p", *a, c), lambda *a, c=c: run("ac_mlp_block_backward_p", *a, c)) for c in (0, 1)]
    torch.cuda.synchronize()
    return out


def layer_legs(M, K, seed=0):
    ref = MU.MLP(K).cuda()
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(M, K, device="cuda", generator=g, requires_grad=K == H)
    go = torch.randn(M, H, device="cuda", generator=g)
    legs = []
    for form in FORMS:
        h = torch.nn.Module()
        h.mlp = MU.MLP(K).cuda()
        h.mlp.load_state_dict(ref.state_dict())
        assert pkg.use_device_mlp(h, products=form) == 1 and h.mlp.products == form

        def fwdbwd(layer=h.mlp):
            (layer(x) * go).sum().backward()
        legs.append(fwdbwd)
    return legs


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
        assert pkg.use_device_gru_layer(pol, products="bf16x3", dense_products="bf16x3") == 2
        assert pkg.use_device_mlp(pol, products=form) == 4 and pkg.use_device_act(pol) == 1
        legs.append(lambda pol=pol: trainer.ppo_update(pol, sample))
    return legs


def accuracy_lines(N=4096, T=60):
    rel = lambda a, ref: float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))
    M = N * T
    inp = S.edge_inputs(M, H)

    def layer(dtype, products=None):
        m = MU.MLP(H).cuda().to(dtype)
        m.load_state_dict({k: torch.as_tensor(inp[k]).to(dtype) for k in MU.PNAMES})
        if products is None:
            return m, MU.module_layer_fn(m)
        fc = m.fc
        return m, lambda x: (lambda y0: (y0, pkg.mlp_block(y0, fc[3], fc[5], products=products)))(pkg.mlp_block(x, fc[0], fc[2], products=products))

    m64, _ = layer(torch.float64)
    with torch.no_grad():
        z0 = m64.fc[0](torch.as_tensor(inp["x"]).to("cuda", torch.float64))
        z1 = m64.fc[3](m64.fc[2](torch.relu(z0)))
        near = ((z0.abs() < 2.0 ** -14).any(1) | (z1.abs() < 2.0 ** -14).any(1)).cpu().numpy()
    del z0, z1
    inp["g_out"][near] = 0.0

    def run(dtype, products=None):
        m, fn = layer(dtype, products)
        x = torch.as_tensor(inp["x"]).to("cuda", dtype).requires_grad_()
        res = MU.run_with_grads(fn, dict(m.named_parameters()), x, torch.as_tensor(inp["g_out"]).to("cuda", dtype))
        torch.cuda.empty_cache()
        return res
    f64 = run(torch.float64)
    res = {"torch fp32": run(torch.float32), "fp32 kernels": run(torch.float32, "fp32"), "split kernels": run(torch.float32, "bf16x3")}
    lines = [f"# errors at {N} x {T}, a two-block layer 128 -> 128 -> 128: rel = max|a - ref| / max|ref| against a float64 torch run; "
             "bound = max(4 x torch fp32, 2^-20)",
             f"# rows left out of the gradients (a |z64| below 2^-14; their upstream gradient is zeroed): {int(near.sum())} of {M} "
             f"({100 * near.mean():.2f} %); the forward results are compared on all rows",
             f"{'key':8s} {'torch fp32':>11} {'fp32 kernels':>13} {'split kernels':>14} {'bound':>10} {'split / bound':>14}"]
    for k in MU.KEYS:
        e = [rel(res[t][k], f64[k]) for t in ("torch fp32", "fp32 kernels", "split kernels")]
        bd = max(4 * e[0], 2.0 ** -20)
        lines.append(f"{k:8s} {e[0]:11.2e} {e[1]:13.2e} {e[2]:14.2e} {bd:10.2e} {e[2] / bd:14.2f}")
    return lines


def trace(N, T, iters=10):
    calls = [block_calls(N * T, K) for K in KS]
    for _ in range(iters):
        for per in calls:
            for form in per:
                form[1](); form[2](); form[3]()
    torch.cuda.synchronize()


def stats_lines(stats_dir):
    lines = ["# rocprofv3 --kernel-trace --stats of the block kernels in both forms (mlpt:: fp32, mlps:: split), a run per shape "
             "(us per launch; forward with the statistics kept)",
             f"{'N':>6} {'T':>3} {'kernel':40s} {'calls':>6} {'avg':>9} {'min':>9} {'max':>9}"]
    found = False
    shape_of = lambda d: tuple(int(v) for v in os.path.basename(d).split("x"))
    for d in sorted(glob.glob(os.path.join(stats_dir, "*x*")), key=lambda d: SHAPES.index(shape_of(d)) if shape_of(d) in SHAPES else len(SHAPES)) if stats_dir else []:
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            continue
        N, T = shape_of(d)
        rows = []
        for row in csv.DictReader(open(files[0])):
            name = row["Name"].replace("void ", "").split("(")[0]
            if "mlp_block_" in name:
                rows.append((name, row))
        for name, row in sorted(rows, key=lambda nr: (nr[0].split("::")[-1].replace("_b3", ""), nr[0])):
            found = True
            lines.append(f"{N:6d} {T:3d} {name:40s} {int(row['Calls']):6d} {float(row['AverageNs']) / 1e3:9.1f} {float(row['MinNs']) / 1e3:9.1f} "
                         f"{float(row['MaxNs']) / 1e3:9.1f}")
    return lines if found else lines[:1] + ["  no trace given"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_split_bench.txt"))
    ap.add_argument("--shapes", default="")
    ap.add_argument("--parent-lib", default="", help="libaircombat_hip.so built from the parent commit, for leg e")
    ap.add_argument("--no-errors", action="store_true", help="skip the error table at 4096 x 60")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it (a second part of the same file)")
    ap.add_argument("--trace", default="", help="NxT: the C calls in both forms at that shape, for a rocprofv3 kernel trace")
    ap.add_argument("--stats", default=None, help="directory of the kernel traces: <stats>/<N>x<T>/**/*kernel_stats.csv")
    a = ap.parse_args()
    if a.trace:
        return trace(*(int(v) for v in a.trace.split("x")))
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")] if a.shapes else SHAPES
    parent = ctypes.CDLL(a.parent_lib) if a.parent_lib else None
    lines = [f"# tools/diag/mlp_split_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {RUNS} consecutive runs, each the "
             f"median of {a.reps} calls per leg (ms), the legs alternating call by call: device = HIP events around each call, wall = per call "
             "with a synchronise"]
    try:
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        rev = ""
    lines.append(f"# {'parent commit ' + rev + ' plus ' if rev else ''}the working tree of this change; fp32 = the parent's kernels, unchanged; "
                 f"split kernels for KP = {[kp for kp in (32, 64, 128, 256) if pkg.load_library().ac_mlp_block_constant(3) & kp]}")
    lines.append(f"{'N':>6} {'T':>3} {'what':66s} {'run':>3} {'fp32 dev':>9} {'bf16x3 dev':>10} {'fp32 wall':>9} {'bf16x3 wall':>11}")
    slower, dev = [], {}
    for N, T in shapes:
        M = N * T
        todo = []
        for K in KS:
            per = block_calls(M, K)
            for i, kind in zip((0, 2, 3), KINDS):
                todo.append((f"a. {kind}, K = {K}", (K, kind), (per[0][i], per[1][i])))
        for K, i, how in ((H, 2, "with dx"), (15, 3, "without dx")):
            per = block_calls(M, K)
            todo.append((f"b. forward + backward calls {how}, K = {K}", None,
                         tuple((lambda f=form[1], bw=form[i]: (f(), bw())) for form in per)))
        for K in (H, 15):
            todo.append((f"c. two-block layer {K} -> 128 -> 128, forward + backward", None, lambda K=K: layer_legs(M, K)))
        todo.append(("d. actor + critic minibatch, DevicePPOTrainer, GRU layer bf16x3", None, lambda: minibatch_legs(N, T)))
        if parent is not None:
            old, new = block_calls(M, H, lib=parent)[0], block_calls(M, H, lib="tree")[0]
            todo.append(("e. default, forward + backward calls with dx, K = 128: parent | this tree", None,
                         ((lambda: (old[1](), old[2]())), (lambda: (new[1](), new[2]())))))
        for what, key, legs in todo:
            fa, fb = legs() if callable(legs) else legs
            for run in range(RUNS):
                (pd, pw), (nd, nw) = timed_pair(fa, fb, a.reps)
                lines.append(f"{N:6d} {T:3d} {what:66s} {run + 1:3d} {pd:9.3f} {nd:10.3f} {pw:9.3f} {nw:11.3f}")
                print(lines[-1], flush=True)
                if nd > pd or nw > pw:
                    slower.append((N, T, what, run + 1))
                if key is not None:
                    dev.setdefault((N, T), {}).setdefault(key, []).append((pd, nd))
            del fa, fb
            torch.cuda.empty_cache()
        del todo
        torch.cuda.empty_cache()
    lines.append("# second column slower than the first (device or wall): " + (", ".join(f"{n} x {t} leg {w.split(':')[0]} run {r}" for n, t, w, r in slower) or "nowhere"))
    kept = {}
    for shape in VERDICT_SHAPES:
        for key, v in dev.get(shape, {}).items():
            s = np.array(v)
            spread = float(max(np.ptp(s[:, 0]), np.ptp(s[:, 1])))
            ok = bool((s[:, 0] - s[:, 1] > spread).all())
            kept[key] = kept.get(key, True) and ok
            lines.append(f"# verdict {shape[0]} x {shape[1]} {key[1]}, K = {key[0]} (KP = {S.split_kp(key[0])}), device ms per run: fp32 "
                         f"{', '.join(f'{x:.3f}' for x in s[:, 0])}; bf16x3 {', '.join(f'{x:.3f}' for x in s[:, 1])}; largest run-to-run spread "
                         f"{spread:.3f}; bf16x3 faster by more than that in every run: {'yes' if ok else 'NO'}")
    for key, ok in kept.items():
        lines.append(f"# condition for keeping the split {key[1]} at KP = {S.split_kp(key[0])}: {'met' if ok else 'NOT met'}")
    if not a.no_errors:
        lines += accuracy_lines()
    lines += stats_lines(a.stats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-60:]))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
