#!/usr/bin/env python3
"""Time evaluation steps run two ways on the same handles: the Python loop of INTEGRATION.md §5d / §5e (act_into_env for both sides,
step_device, the runners' eval() bookkeeping in torch: dones_env, cumulative rewards, the episode log, zeroed GRU rows, masks) and
DeviceEvaluator.begin(); run(n). The loop uses only calls that were there before the evaluator, so it is the
baseline. Shapes, at 4096 envs: BASELINE 1v1 (singlecombat) self-play against one actor-only policy, 2v2 (multiplecombat) self-play
against a PPO-form pool of 3, and the hierarchical 4v4 scenario (scenario3_nvn) in self-play against a mappo-form pool of 3.

Per shape, `--reps` runs; within each run the two paths alternate, `--steps` steps of each, after one warm-up of each. us per step:
'wall' = host clock around the steps and a device synchronise; 'stream' = HIP events on torch's stream around the same (for run(): the
device time of the steps, which the call orders on that stream). Median and min .. max over the runs. 'kernels' = the per-step kernels'
own average times from a rocprofv3 kernel trace of run(), taken in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/<shape> -- python tools/diag/eval_bench.py --trace --shape <shape>
    python tools/diag/eval_bench.py --stats OUT          # the timed run; writes profiles/eval_bench.txt
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
# shape: (task, hierarchical, MAPPO form, opponent: "policy" / "pool")
SHAPES = {"baseline_1v1_selfplay": ("singlecombat", False, False, "policy"), "mc_2v2_selfplay_pool3": ("multiplecombat", False, False, "pool"),
          "scenario3_4v4_hier_mappo_pool3": ("scenario3_nvn", True, True, "pool")}
TRACE_RUNS = 4
K = 4
POST_KERNEL = "eval_post_kernel"


def state_dicts(obs_dim, cent_dim, nvec, n_shoot, seed):
    a = U.seeded_state_dicts(obs_dim, nvec, True, seed=seed)[0]
    c = U.seeded_state_dicts(cent_dim, nvec, True, seed=seed)[1]
    for s in range(n_shoot):
        k = len(nvec) + s
        a[f"act.action_outs.{k}.net.weight"] = (U.hashed(seed * 1000 + 300 + s, 256) / np.sqrt(128)).reshape(2, 128).astype(np.float32)
        a[f"act.action_outs.{k}.net.bias"] = (U.hashed(seed * 1000 + 400 + s, 2) / np.sqrt(128)).astype(np.float32)
    return a, c


class Handles:
    def __init__(self, shape, E, T):
        task, hier, mappo, opp_kind = SHAPES[shape]
        self.env = env = (pkg.HipShareVecEnv if mappo else pkg.HipVecEnv)(pkg.default_config(task, hierarchical=hier), E, device_id=0, seed=1)
        self.E, self.T, self.A, self.D = E, T, env.num_agents, env.obs_dim
        A, D = self.A, self.D
        self.na = na = A // 2
        nvec, n_shoot, _ = P._action_heads(env.action_space)
        a = types.SimpleNamespace(hidden_size="128 128", act_hidden_size="128 128", recurrent_hidden_size=128, recurrent_hidden_layers=1,
                                  activation_id=1, use_feature_normalization=True, use_prior=n_shoot > 0, use_recurrent_policy=True)
        if mappo:
            cent = env.share_observation_space
            make = lambda seed: P.DeviceMAPPOPolicy(env.observation_space, cent, env.action_space, a, seed=seed, critic=False)
        else:
            make = lambda seed: P.DevicePolicy(env.observation_space, env.action_space, a, seed=seed, critic=False)
        self.policy = make(3)
        self.policy.load_state_dict(state_dicts(D, A * D, nvec, n_shoot, 50)[0])
        if opp_kind == "pool":
            self.opp = P.DevicePolicyPool(env.observation_space, env.action_space, a, 3, form="mappo" if mappo else "ppo", seed=4)
            for k in range(3):
                self.opp.load_state_dict(k, state_dicts(D, A * D, nvec, n_shoot, 60 + k)[0])
            self.opp.assign_split(E, [0, 1, 2], na=A - na)
        else:
            self.opp = make(4)
            self.opp.load_state_dict(state_dicts(D, A * D, nvec, n_shoot, 60)[0])
        env.reset()
        self.start = env.snapshot()                  # every timed run starts from this state, so the two paths' logs can be compared
        self.ev = pkg.DeviceEvaluator(env, self.policy, opponent=self.opp, num_learner_agents=na, episodes_per_env=K)
        # the loop's own evaluation state
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
        self.h, self.m = z(E * na, 1, 128), z(E * na, 1)
        self.h_opp, self.m_opp = z(E * (A - na), 1, 128), z(E * (A - na), 1)
        self.cum, self.len, self.count = z(E, A), z(E, dt=torch.int32), z(E, dt=torch.int32)
        self.log_ret, self.log_len, self.log_end = z(E, K, A), z(E, K, dt=torch.int32), z(E, K, dt=torch.int32)
        self.remaining = z(1, dt=torch.int32)

    def python_loop(self):
        """begin and T steps; the bookkeeping stays on the device (no host wait beyond what the calls themselves need)"""
        env, pol, na, A, E = self.env, self.policy, self.na, self.A, self.E
        _, _, rew, done, _ = env.device_tensors()
        cur = torch.cuda.current_stream()
        for t in (self.h, self.h_opp, self.cum, self.len, self.count, self.log_ret, self.log_len, self.log_end):
            t.zero_()
        self.m.fill_(1.0)
        self.m_opp.fill_(1.0)
        self.remaining.fill_(E)
        env_idx = torch.arange(E, device="cuda")
        for t in range(self.T):
            pol.act_into_env(env, self.h, self.m, agents=slice(0, na), deterministic=True)
            self.opp.act_into_env(env, self.h_opp, self.m_opp, agents=slice(na, A), deterministic=True)
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
            self.remaining -= (write & (self.count == K - 1)).sum().to(torch.int32)
            self.count += dones_env.to(torch.int32)
            self.cum *= keep[:, None]
            self.len *= (~dones_env).to(torch.int32)
            self.h.view(E, na, 128).mul_(keep[:, None, None])
            self.h_opp.view(E, A - na, 128).mul_(keep[:, None, None])
            self.m.copy_(keep[:, None].expand(E, na).reshape(-1, 1))
            self.m_opp.copy_(keep[:, None].expand(E, A - na).reshape(-1, 1))

    def run(self):
        self.ev.begin()
        self.ev.run(self.T)

    def timed(self, fn):
        self.env.restore(self.start)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        self.env.sync()
        return wall * 1e6 / self.T, e0.elapsed_time(e1) * 1e3 / self.T

    def close(self):
        for x in (self.ev, self.opp, self.policy, self.env):
            x.close()


def kernel_sum(stats_dir, shape, steps):
    """(sum of average ns per step, [(name, calls per step, average ns)]) of the kernels launched every step in the trace of `shape`."""
    files = glob.glob(os.path.join(stats_dir, shape, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None, []
    rows = []
    for r in csv.DictReader(open(files[0])):
        per = int(r["Calls"]) / steps
        if per >= 1 and abs(per - round(per)) < 1e-9:
            rows.append((r["Name"].split("(")[0].replace("void ", ""), int(round(per)), float(r["AverageNs"])))
    return sum(n * a for _, n, a in rows), rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", default=None)
    ap.add_argument("--trace", action="store_true", help="run() only, for a rocprofv3 kernel trace of one shape")
    ap.add_argument("--stats", default=None, help="directory of the kernel traces: <stats>/<shape>/**/*kernel_stats.csv")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.txt"))
    a = ap.parse_args()
    shapes = [a.shape] if a.shape else list(SHAPES)
    if a.trace:
        for shape in shapes:
            h = Handles(shape, a.envs, a.steps)
            for _ in range(TRACE_RUNS):
                h.timed(h.run)
            h.close()
        return
    fmt = lambda x: f"{np.median(x):8.1f} ({min(x):.1f} .. {max(x):.1f})"
    lines = [f"# {a.steps} evaluation steps at {a.envs} envs, {K} log slots per env, the Python loop of INTEGRATION.md 5d / 5e vs "
             f"DeviceEvaluator.begin(); run({a.steps}) on the same handles, {torch.cuda.get_device_name(0)}; {a.reps} runs, the two paths "
             "alternating within each, after one warm-up of each. us per step, median (min .. max): wall = host clock around the steps + "
             "synchronise; stream = HIP events on torch's stream around them. kernels = the per-step kernels' own average times, summed, "
             "from a rocprofv3 kernel trace of run() ONLY (a run of its own; a kernel counts as per-step when its calls are a whole "
             "multiple of the traced steps). post-step = eval_post_kernel's own average time from that trace."]
    for shape in shapes:
        first = len(lines) if shape != shapes[0] else 0
        h = Handles(shape, a.envs, a.steps)
        res = {"python loop": ([], []), "run": ([], [])}
        for rep in range(a.reps + 1):
            for name, fn in (("python loop", h.python_loop), ("run", h.run)):
                w, s = h.timed(fn)
                if rep:
                    res[name][0].append(w)
                    res[name][1].append(s)
        # both paths end on the same log (the same steps from the same env state)
        torch.cuda.synchronize()
        same = all(torch.equal(h.ev.view(k), t) for k, t in (("log_returns", h.log_ret), ("log_lengths", h.log_len), ("counts", h.count),
                                                            ("cum", h.cum), ("remaining", h.remaining)))
        lines.append(f"{shape}: {h.E} envs x {h.A} agents, learner rows {h.E * h.na}, opponent rows {h.E * (h.A - h.na)}, obs {h.D}; "
                     f"episodes finished {int(h.count.sum())}, envs still short of their quota {int(h.remaining)}; the two paths' logs "
                     f"{'agree' if same else 'DIFFER'}")
        for name, (w, s) in res.items():
            lines.append(f"  {name:>12}  wall {fmt(w)}  stream {fmt(s)}  steps/s {1e6 / np.median(w):9.0f}")
        lines.append(f"  {'speed-up':>12}  wall x{np.median(res['python loop'][0]) / np.median(res['run'][0]):.2f}")
        if a.stats:
            tot, rows = kernel_sum(a.stats, shape, TRACE_RUNS * a.steps)
            if tot is None:
                lines.append("  kernels: no trace found")
            else:
                gap = np.median(res["run"][1]) - tot / 1e3
                lines.append(f"  {'kernels':>12}  {tot / 1e3:8.1f} us per step; run's stream time leaves {gap:.1f} us per step between them")
                for name, n, avg in rows:
                    lines.append(f"      {n} x {avg / 1e3:7.1f} us  {name[:110]}")
                post = [avg for name, _, avg in rows if POST_KERNEL in name]
                if post:
                    lines.append(f"  {'post-step':>12}  {post[0] / 1e3:7.1f} us")
        else:
            lines.append("  kernels: no trace given")
        print("\n".join(lines[first:]), flush=True)
        h.close()
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(txt)


if __name__ == "__main__":
    main()
