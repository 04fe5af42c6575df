#!/usr/bin/env python3
"""Time league steps run two ways on the same handles: DeviceLeague.begin(); run(n) and the stepwise Python loop
of the same launches (pool.act_into_env over every agent under the sided plan, step_device, the bookkeeping in torch). Shapes, at
4096 envs with a pool of 4 dealt by round_robin: BASELINE 1v1 (singlecombat) and the hierarchical 2v2 scenario (scenario2_nvn).

Per shape, `--reps` runs; within each run the two legs alternate, `--steps` steps of each, after one warm-up of each. us per step:
'wall' = host clock around the steps and a device synchronise; 'stream' = HIP events on torch's stream around the same. Median and
min .. max over the runs. The table() call is timed the same way after the last run. 'kernels' = the per-step kernels' own average
times, and the two table kernels', from a rocprofv3 kernel trace of run() and table(), taken in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/<shape> -- python tools/diag/league_bench.py --trace --shape <shape>
    python tools/diag/league_bench.py --stats OUT          # the timed run; writes profiles/league_bench.txt
"""
import argparse
import csv
import glob
import importlib
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
torch.cuda.init()
import aircombat_selfplay_amd as pkg  # noqa: E402
import policy_util as U  # noqa: E402

P = importlib.import_module("aircombat-selfplay_amd.policy")
# shape: (task, hierarchical)
SHAPES = {"baseline_1v1_pool4": ("singlecombat", False), "scenario2_2v2_hier_pool4": ("scenario2_nvn", True)}
TRACE_RUNS = 4
K, CAP = 4, 4
POST_KERNEL, TABLE_KERNELS = "league_post_kernel", ("league_partial_kernel", "league_cells_kernel")


class Handles:
    def __init__(self, shape, E, T):
        task, hier = SHAPES[shape]
        cfg = pkg.default_config(task, hierarchical=hier)
        probe = pkg.HipVecEnv(cfg, 1, device_id=0, seed=1)
        wide = probe.obs_dim > 32          # the PPO form's actor takes observations up to 32 wide; wider ones go to mappo-form members
        probe.close()
        self.env = env = (pkg.HipShareVecEnv if wide else pkg.HipVecEnv)(cfg, E, device_id=0, seed=1)
        self.E, self.T, self.A, self.D, self.form = E, T, env.num_agents, env.obs_dim, "mappo" if wide else "ppo"
        nvec, n_shoot, _ = P._action_heads(env.action_space)
        a = types.SimpleNamespace(hidden_size="128 128", act_hidden_size="128 128", recurrent_hidden_size=128, recurrent_hidden_layers=1,
                                  activation_id=1, use_feature_normalization=True, use_prior=n_shoot > 0, use_recurrent_policy=True)
        self.pool = P.DevicePolicyPool(env.observation_space, env.action_space, a, CAP, form=self.form, seed=4)
        for k in range(CAP):
            self.pool.load_state_dict(k, U.add_munition_heads(U.seeded_state_dicts(self.D, nvec, True, seed=60 + k)[0], len(nvec), n_shoot, 60 + k))
        self.pool.assign_sides(pkg.round_robin(E, range(CAP)), self.A)
        env.reset()
        self.start = env.snapshot()                  # every timed run starts from this state, so the two legs' logs can be compared
        self.lg = pkg.DeviceLeague(env, self.pool, episodes_per_env=K)
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
        A = self.A
        self.h, self.m = z(E * A, 1, 128), z(E * A, 1)
        self.cum, self.len, self.count = z(E, A), z(E, dt=torch.int32), z(E, dt=torch.int32)
        self.log_ret = z(E, K, A)
        self.log_len, self.log_end, self.log_code = (z(E, K, dt=torch.int32) for _ in range(3))
        self.remaining = z(1, dt=torch.int32)

    def python_loop(self):
        """begin and T steps; the bookkeeping stays on the device (no host wait beyond what the calls themselves need)"""
        env, pool, A, E = self.env, self.pool, self.A, self.E
        _, _, rew, done, info = env.device_tensors()
        cur = torch.cuda.current_stream()
        for t in (self.h, self.cum, self.len, self.count, self.log_ret, self.log_len, self.log_end, self.log_code):
            t.zero_()
        self.m.fill_(1.0)
        self.remaining.fill_(E)
        env_idx = torch.arange(E, device="cuda")
        for t in range(self.T):
            pool.act_into_env(env, self.h, self.m, agents=slice(0, A))
            env.step_device(stream=cur)
            dones_env = done.reshape(E, A).bool().all(dim=1)
            keep = (~dones_env).float()
            self.cum += rew.reshape(E, A)
            self.len += 1
            write = dones_env & (self.count < K)
            slot = self.count.clamp(max=K - 1).long()
            self.log_ret[env_idx, slot] = torch.where(write[:, None], self.cum, self.log_ret[env_idx, slot])
            self.log_len[env_idx, slot] = torch.where(write, self.len, self.log_len[env_idx, slot])
            self.log_end[env_idx, slot] = torch.where(write, torch.full_like(self.len, t), self.log_end[env_idx, slot])
            self.log_code[env_idx, slot] = torch.where(write, info.reshape(E, 4)[:, 1], self.log_code[env_idx, slot])
            self.remaining -= (write & (self.count == K - 1)).sum().to(torch.int32)
            self.count += dones_env.to(torch.int32)
            self.cum *= keep[:, None]
            self.len *= (~dones_env).to(torch.int32)
            self.h.view(E, A, 128).mul_(keep[:, None, None])
            self.m.copy_(keep[:, None].expand(E, A).reshape(-1, 1))

    def run(self):
        self.lg.begin()
        self.lg.run(self.T)

    def timed(self, fn, restore=True, per=None):
        if restore:
            self.env.restore(self.start)
            self.pool.counter = 0                    # both legs draw the same numbers
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        self.env.sync()
        per = per or self.T
        return wall * 1e6 / per, e0.elapsed_time(e1) * 1e3 / per

    def close(self):
        for x in (self.lg, self.pool, self.env):
            x.close()


def kernel_rows(stats_dir, shape):
    """[(name, calls, average ns)] of the trace of `shape`, or None"""
    files = glob.glob(os.path.join(stats_dir, shape, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None
    return [(r["Name"].split("(")[0].replace("void ", ""), int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(open(files[0]))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", default=None)
    ap.add_argument("--trace", action="store_true", help="run() and table() only, for a rocprofv3 kernel trace of one shape")
    ap.add_argument("--stats", default=None, help="directory of the kernel traces: <stats>/<shape>/**/*kernel_stats.csv")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "league_bench.txt"))
    a = ap.parse_args()
    shapes = [a.shape] if a.shape else list(SHAPES)
    if a.trace:
        for shape in shapes:
            h = Handles(shape, a.envs, a.steps)
            for _ in range(TRACE_RUNS):
                h.timed(h.run)
                h.lg.table()
            h.close()
        return
    fmt = lambda x: f"{np.median(x):8.1f} ({min(x):.1f} .. {max(x):.1f})"
    lines = [f"# {a.steps} league steps at {a.envs} envs, a pool of {CAP} dealt by round_robin, {K} log slots per env: "
             f"DeviceLeague.begin(); run({a.steps}) vs the stepwise Python loop of the same launches (pool.act_into_env over every agent, "
             f"step_device, torch bookkeeping) on the same handles, {torch.cuda.get_device_name(0)}; {a.reps} runs, the two legs "
             "alternating within each, after one warm-up of each. us per step, median (min .. max): wall = host clock around the steps + "
             "synchronise; stream = HIP events on torch's stream around them. table = one table() call (two kernels and the copy of the "
             "cells), us per call. kernels = the per-step kernels' own average times, summed, from a rocprofv3 kernel trace of run() and "
             "table() ONLY (a run of its own; a kernel counts as per-step when its calls are a whole multiple of the traced steps)."]
    for shape in shapes:
        first = len(lines) if shape != shapes[0] else 0
        h = Handles(shape, a.envs, a.steps)
        res = {"run": ([], []), "python loop": ([], [])}
        for rep in range(a.reps + 1):
            for name, fn in (("run", h.run), ("python loop", h.python_loop)):
                w, s = h.timed(fn)
                if rep:
                    res[name][0].append(w)
                    res[name][1].append(s)
        # both legs end on the same log (the same steps from the same env state with the same draws)
        torch.cuda.synchronize()
        same = all(torch.equal(h.lg.view(k), t) for k, t in (("log_returns", h.log_ret), ("log_lengths", h.log_len), ("log_codes", h.log_code),
                                                            ("counts", h.count), ("cum", h.cum), ("remaining", h.remaining)))
        tab = [h.timed(h.lg.table, restore=False, per=1) for _ in range(a.reps + 1)][1:]
        t = h.lg.table()
        lines.append(f"{shape}: {h.E} envs x {h.A} agents ({h.form} form), rows {h.E * h.A}, obs {h.D}; episodes finished {int(h.count.sum())}, "
                     f"in the table {int(t.episodes.sum())} over {int((t.episodes > 0).sum())} cells, envs still short of their quota "
                     f"{int(h.remaining)}; the two legs' logs {'agree' if same else 'DIFFER'}")
        for name, (w, s) in res.items():
            lines.append(f"  {name:>12}  wall {fmt(w)}  stream {fmt(s)}  steps/s {1e6 / np.median(w):9.0f}")
        lines.append(f"  {'speed-up':>12}  wall x{np.median(res['python loop'][0]) / np.median(res['run'][0]):.2f}")
        lines.append(f"  {'table':>12}  wall {fmt([w for w, _ in tab])}  stream {fmt([s for _, s in tab])}")
        rows = kernel_rows(a.stats, shape) if a.stats else None
        if rows is None:
            lines.append("  kernels: no trace " + ("found" if a.stats else "given"))
        else:
            steps = TRACE_RUNS * a.steps
            per_step = [(n, c // steps, avg) for n, c, avg in rows if c >= steps and c % steps == 0]
            tot = sum(c * avg for _, c, avg in per_step)
            lines.append(f"  {'kernels':>12}  {tot / 1e3:8.1f} us per step; run's stream time leaves "
                         f"{np.median(res['run'][1]) - tot / 1e3:.1f} us per step between them")
            for n, c, avg in per_step:
                lines.append(f"      {c} x {avg / 1e3:7.1f} us  {n[:110]}")
            for want in (POST_KERNEL,) + TABLE_KERNELS:
                got = [avg for n, _, avg in rows if want in n]
                if got:
                    lines.append(f"  {want:>24}  {got[0] / 1e3:7.1f} us")
        print("\n".join(lines[first:]), flush=True)
        h.close()
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(txt)


if __name__ == "__main__":
    main()
