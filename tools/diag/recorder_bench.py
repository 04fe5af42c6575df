#!/usr/bin/env python3
"""What the flight recorder costs an evaluation, and what it replaces. All runs at 4096 envs.

1. DeviceEvaluator.begin(); run(256) on eval_bench.py's handles (BASELINE 1v1 self-play against one policy, and the hierarchical 4v4
   scenario against a mappo pool of 3) three ways: no recorder attached, a recorder on 16 envs, a recorder on all envs. `--reps` runs;
   within each run the three alternate, after one warm-up of each. us per step: 'wall' = host clock around the steps and a device
   synchronise; 'stream' = HIP events on torch's stream around the same. Median and min .. max over the runs.
2. The capture kernel's own average time from a rocprofv3 kernel trace of run() with the recorder attached, taken in runs of their own,
   and the bytes it writes per capture:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/<shape>_<leg> -- python tools/diag/recorder_bench.py --trace --shape <shape> --leg <16|all>
    python tools/diag/recorder_bench.py --stats OUT          # the timed run; writes profiles/recorder_bench.txt

3. What the recorder replaces for one env: the stepwise loop step_device(); render() over 256 steps at the same 4096 envs (render() reads
   the env through blocking host getters), next to frames() + write_acmi() of the same 256 steps from the ring.
"""
import argparse
import csv
import glob
import os
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import eval_bench as EB  # noqa: E402  (the evaluator's handles and its timing bracket)

pkg, ROOT = EB.pkg, EB.ROOT
SHAPES = ["baseline_1v1_selfplay", "scenario3_4v4_hier_mappo_pool3"]
LEGS = ["none", "16", "all"]
TRACE_RUNS = 4
CAPTURE_KERNEL = "recorder_capture_kernel"


def selection(leg, E):
    return None if leg == "all" else [int(e) for e in np.linspace(0, E - 1, 16).astype(int)]


class Legs:
    """eval_bench's handles with one recorder per leg; attach(leg) swaps the attached one"""

    def __init__(self, shape, E, T, legs=LEGS):
        self.h = EB.Handles(shape, E, T)
        self.recs = {leg: pkg.FlightRecorder(self.h.env, envs=selection(leg, E), frames=T) for leg in legs if leg != "none"}

    def attach(self, leg):
        self.h.env.stop_recording()
        if leg != "none":
            self.recs[leg].attach()

    def close(self):
        self.h.close()


def capture_time(stats_dir, shape, leg):
    files = glob.glob(os.path.join(stats_dir, f"{shape}_{leg}", "**", "*kernel_stats.csv"), recursive=True)
    for r in (csv.DictReader(open(files[0])) if files else []):
        if CAPTURE_KERNEL in r["Name"]:
            return int(r["Calls"]), float(r["AverageNs"])
    return None


def render_loop(E, T):
    """step_device + render() for one env, and the recorder's way to the same file, on a BASELINE 1v1 handle of E envs"""
    env = pkg.HipVecEnv(pkg.default_config("singlecombat"), E, device_id=0, seed=1)
    env.reset()
    start = env.snapshot()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name in ("render", "recorder"):
            env.restore(start)
            rec = env.record(envs=[E // 2], frames=T) if name == "recorder" else None
            env.sync()
            t0 = time.perf_counter()
            for _ in range(T):
                env.step_device()
                if rec is None:
                    env.render(filepath=os.path.join(d, "render.acmi"), env=E // 2)
            if rec is not None:
                rec.write_acmi(os.path.join(d, "rec.acmi"), E // 2)
            env.sync()
            out[name] = (time.perf_counter() - t0) * 1e6 / T
        same = open(os.path.join(d, "render.acmi"), "rb").read() == open(os.path.join(d, "rec.acmi"), "rb").read()
    env.close()
    return out, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", default=None)
    ap.add_argument("--leg", default="all", choices=LEGS[1:])
    ap.add_argument("--trace", action="store_true", help="run() with one recorder attached only, for a rocprofv3 kernel trace")
    ap.add_argument("--stats", default=None, help="directory of the kernel traces: <stats>/<shape>_<leg>/**/*kernel_stats.csv")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recorder_bench.txt"))
    a = ap.parse_args()
    shapes = [a.shape] if a.shape else SHAPES
    if a.trace:
        for shape in shapes:
            L = Legs(shape, a.envs, a.steps, legs=[a.leg])
            L.attach(a.leg)
            for _ in range(TRACE_RUNS):
                L.h.timed(L.h.run)
            L.close()
        return
    fmt = lambda x: f"{np.median(x):8.1f} ({min(x):.1f} .. {max(x):.1f})"
    lines = [f"# DeviceEvaluator.begin(); run({a.steps}) at {a.envs} envs with no flight recorder, a recorder on 16 envs and a recorder on all "
             f"envs (ring of {a.steps} frames), {torch.cuda.get_device_name(0)}; {a.reps} runs, the three legs alternating within each, after "
             "one warm-up of each. us per step, median (min .. max): wall = host clock around the steps + synchronise; stream = HIP events "
             "on torch's stream around them. capture = recorder_capture_kernel's own average time from a rocprofv3 kernel trace taken in a "
             "run of its own, and the bytes it writes per capture (selected aircraft x bytes per aircraft-frame)."]
    for shape in shapes:
        first = len(lines) if shape != shapes[0] else 0
        L = Legs(shape, a.envs, a.steps)
        h = L.h
        res = {leg: ([], []) for leg in LEGS}
        for rep in range(a.reps + 1):
            for leg in LEGS:
                L.attach(leg)
                w, s = h.timed(h.run)
                if rep:
                    res[leg][0].append(w)
                    res[leg][1].append(s)
        lines.append(f"{shape}: {h.E} envs x {h.A} agents, {L.recs['all'].bytes_per_aircraft_frame} B per aircraft-frame; rings "
                     f"{L.recs['16'].nbytes / 2**20:.1f} MiB (16 envs) and {L.recs['all'].nbytes / 2**20:.1f} MiB (all envs)")
        base = np.median(res["none"][1])
        for leg in LEGS:
            w, s = res[leg]
            lines.append(f"  {'recorder ' + leg:>14}  wall {fmt(w)}  stream {fmt(s)}  stream vs none {np.median(s) - base:+6.1f} us")
        for leg in LEGS[1:]:
            got = capture_time(a.stats, shape, leg) if a.stats else None
            rec = L.recs[leg]
            nbytes = len(rec.envs) * h.A * rec.bytes_per_aircraft_frame
            if got is None:
                lines.append(f"  capture ({leg}): no trace given; {nbytes} B written per capture")
            else:
                calls, avg = got
                lines.append(f"  capture ({leg}): {avg / 1e3:6.2f} us average over {calls} captures; {nbytes} B written per capture = "
                             f"{nbytes / avg:.1f} GB/s of stores")
        print("\n".join(lines[first:]), flush=True)
        L.close()
    if not a.shape:
        first = len(lines)
        t, same = render_loop(a.envs, a.steps)
        lines.append(f"one env's ACMI file over {a.steps} steps at {a.envs} envs (BASELINE 1v1), us per step of wall time: step_device + render() "
                     f"{t['render']:.1f}; step_device with a recorder on that env, then write_acmi {t['recorder']:.1f}; the two files "
                     f"{'are equal' if same else 'DIFFER'}")
        print("\n".join(lines[first:]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
