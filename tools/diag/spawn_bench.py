#!/usr/bin/env python3
"""What a spawn curriculum costs a device-resident step. All runs at 4096 envs, max_steps = 100 so that respawns
(every env, every 100th step) are inside the timed steps.

1. step_device on the hierarchical scenario1 task (1v1) and the hierarchical 2v2 scenario three ways: nothing attached, a bank of the
   reference's 181 angles with mode="fixed" (stages spread over the bank), and the same bank with mode="auto", sample="upto". `--reps`
   runs; within each run the three alternate, after one warm-up of each. us per step of stream time: HIP events on the handle's stream
   around `--steps` steps (ac_timing_begin / ac_timing_end). Median and min .. max over the runs.
2. The nothing-attached leg against another checkout of the package (the parent commit) in the same session:

    python tools/diag/spawn_bench.py --parent-root PATH     # PATH: a built checkout

   Both checkouts' nothing-attached legs then run in `--reps` processes of their own each, alternating (a process's figure is the
   median of its `--reps` runs; runs inside one process agree to a few hundredths of a us, processes differ by more). The leg is
   unchanged when the two medians over the processes differ by no more than the parent's own min .. max spread over its processes.
3. The spawn kernel's own average time from a rocprofv3 kernel trace, taken in runs of their own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/<shape>_<leg> -- python tools/diag/spawn_bench.py --trace --shape <shape> --leg <fixed|auto_upto>
    python tools/diag/spawn_bench.py --stats OUT            # the timed run; writes profiles/spawn_bench.txt
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = {"scenario1_1v1_hier": "scenario1", "scenario2_2v2_hier": "scenario_nvn"}
LEGS = ["none", "fixed", "auto_upto"]
SPAWN_KERNEL = "spawn_kernel"


def handle(pkg, shape, E):
    import torch
    cfg = pkg.default_config(SHAPES[shape], hierarchical=True)
    cfg.max_steps = 100
    env = pkg.HipVecEnv(cfg, E, device_id=0, seed=1)
    env.reset()
    act = env.device_tensors()[0]
    g = torch.Generator(device="cuda").manual_seed(3)
    for k, n in enumerate((3, 5, 3, 2, 2, 2, 2)):
        act[..., k] = torch.randint(0, n, act.shape[:2], generator=g, device="cuda").float()
    torch.cuda.synchronize()
    return env


def attach(env, leg):
    import torch
    env.stop_curriculum()
    if leg == "none":
        return
    kw = dict(mode="auto", sample="upto", win_return=0.0, seed=5) if leg == "auto_upto" else {}
    cur = env.spawn_curriculum(angles=range(181), **kw)
    cur.stage.copy_(torch.arange(env.num_envs, dtype=torch.int32, device="cuda") % 181)
    torch.cuda.synchronize()


def stream_us(env, steps):
    lib = env.lib
    lib.check(lib.ac_timing_begin(env._h), "ac_timing_begin")
    for _ in range(steps):
        env.step_device()
    ms = C.c_float()
    lib.check(lib.ac_timing_end(env._h, C.byref(ms)), "ac_timing_end")
    return ms.value * 1e3 / steps


def kernel_time(stats_dir, shape, leg):
    files = glob.glob(os.path.join(stats_dir, f"{shape}_{leg}", "**", "*kernel_stats.csv"), recursive=True)
    for r in (csv.DictReader(open(files[0])) if files else []):
        if SPAWN_KERNEL in r["Name"]:
            return int(r["Calls"]), float(r["AverageNs"])
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", default=None, choices=list(SHAPES))
    ap.add_argument("--leg", default="fixed", choices=LEGS[1:])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(HERE)), help="the checkout whose package is timed (default: this one)")
    ap.add_argument("--none-only", action="store_true", help="the nothing-attached leg alone, as one JSON line (uses nothing newer than step_device)")
    ap.add_argument("--parent-root", default=None, help="another built checkout whose nothing-attached leg is timed in a process of its own")
    ap.add_argument("--trace", action="store_true", help="steps with one bank attached only, for a rocprofv3 kernel trace")
    ap.add_argument("--stats", default=None, help="directory of the kernel traces: <stats>/<shape>_<leg>/**/*kernel_stats.csv")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    torch.cuda.init()
    import aircombat_selfplay_amd as pkg
    shapes = [a.shape] if a.shape else list(SHAPES)
    if a.none_only:
        res = {}
        for shape in shapes:
            env = handle(pkg, shape, a.envs)
            res[shape] = [stream_us(env, a.steps) for _ in range(a.reps + 1)][1:]
            env.close()
        print(json.dumps(res), flush=True)
        return
    if a.trace:
        for shape in shapes:
            env = handle(pkg, shape, a.envs)
            attach(env, a.leg)
            for _ in range(2):
                stream_us(env, a.steps)
            env.close()
        return
    parent = here = None
    if a.parent_root:
        def process(root):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--none-only", "--envs", str(a.envs), "--steps", str(a.steps),
                                  "--reps", str(a.reps)], capture_output=True, text=True, check=True).stdout
            return {k: float(np.median(v)) for k, v in json.loads(out.strip().splitlines()[-1]).items()}
        parent, here = {k: [] for k in SHAPES}, {k: [] for k in SHAPES}
        for _ in range(a.reps):
            for res, root in ((parent, a.parent_root), (here, a.root)):
                for k, v in process(root).items():
                    res[k].append(v)
    fmt = lambda x: f"{np.median(x):8.2f} ({min(x):.2f} .. {max(x):.2f})"
    lines = [f"# step_device at {a.envs} envs, max_steps 100, with nothing attached, a spawn bank of 181 angles in mode='fixed' (stages spread over the "
             f"bank) and the same bank in mode='auto', sample='upto'; {torch.cuda.get_device_name(0)}; {a.reps} runs of {a.steps} steps, the three legs "
             "alternating within each, after one warm-up of each. us per step of stream time (HIP events on the handle's stream), median "
             "(min .. max). spawn_kernel = its own average time from a rocprofv3 kernel trace taken in a run of its own."]
    for shape in shapes:
        first = len(lines) if shape != shapes[0] else 0
        env = handle(pkg, shape, a.envs)
        res = {leg: [] for leg in LEGS}
        for rep in range(a.reps + 1):
            for leg in LEGS:
                attach(env, leg)
                us = stream_us(env, a.steps)
                if rep:
                    res[leg].append(us)
        lines.append(f"{shape}: {env.num_envs} envs x {env.num_agents} agents")
        base = np.median(res["none"])
        for leg in LEGS:
            lines.append(f"  {leg:>10}  stream {fmt(res[leg])}  vs none {np.median(res[leg]) - base:+6.2f} us")
        if parent is None:
            lines.append("  parent commit: not measured (no --parent-root given)")
        else:
            p, q = parent[shape], here[shape]
            ok = abs(np.median(p) - np.median(q)) <= max(p) - min(p)
            lines.append(f"  nothing attached, {len(p)} processes of their own each, alternating: parent commit {fmt(p)}, this checkout {fmt(q)}; the medians differ "
                         f"by {np.median(q) - np.median(p):+.2f} us, {'within' if ok else 'OUTSIDE'} the parent's own spread of {max(p) - min(p):.2f} us")
        for leg in LEGS[1:]:
            got = kernel_time(a.stats, shape, leg) if a.stats else None
            lines.append(f"  spawn_kernel ({leg}): " + ("no trace given" if got is None else f"{got[1] / 1e3:6.2f} us average over {got[0]} launches"))
        print("\n".join(lines[first:]), flush=True)
        env.close()
    out = a.out or os.path.join(os.path.abspath(a.root), "profiles", "spawn_bench.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    open(out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
