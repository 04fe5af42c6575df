#!/usr/bin/env python3
"""Time a whole MAPPO rollout collected two ways on the same handles: the Python loop of INTEGRATION.md §5e (get_actions on the
buffer's share_obs / obs slots, the actions into the env's action buffer, the opponent's act_into_env, step_device, the share runner's
dones_env / masks / active_masks and share_obs in torch, buffer.insert(on_device=True)) and DeviceMAPPORollout.collect (INTEGRATION.md
§5j). The loop uses only calls that were there before the collector, so it is the baseline. Shapes, at 4096 envs: 2v2 MultipleCombat
with the learner on every agent, 2v2 self-play against a mappo pool of 3, and the hierarchical 4v4 scenario (scenario3_nvn) in self-play
against one actor-only opponent.

Per shape, `--reps` rollouts of `--steps` steps of each path, alternating, after one warm-up rollout of each. us per step: 'wall' =
host clock around the rollout and a device synchronise; 'stream' = HIP events on torch's stream around the same (for collect: the
device time of the rollout, which the call orders on that stream; for the loop, which synchronises every step, about the wall time).
Median and min .. max over the rollouts. 'kernels' = the per-step kernels' own average times from a rocprofv3 kernel trace of collect,
taken in a run of its own; the post-step kernel's line adds the bytes it moves per step and their rate as a share of the HBM peak:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/<shape> -- python tools/diag/mappo_rollout_bench.py --trace --shape <shape>
    python tools/diag/mappo_rollout_bench.py --stats OUT          # the timed run; writes profiles/mappo_rollout_bench.txt
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
# shape: (task, hierarchical, opponent: None / "pool" / "policy")
SHAPES = {"mc_2v2_all": ("multiplecombat", False, None), "mc_2v2_selfplay_pool3": ("multiplecombat", False, "pool"),
          "scenario3_4v4_hier_selfplay": ("scenario3_nvn", True, "policy")}
TRACE_ROLLOUTS = 4
HBM_PEAK = 8.0e12      # bytes per second, MI355X
POST_KERNEL = "rollout_share_post_kernel"


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
        task, hier, opp_kind = SHAPES[shape]
        self.env = env = pkg.HipShareVecEnv(pkg.default_config(task, hierarchical=hier), E, device_id=0, seed=1)
        self.E, self.T, self.A, self.D = E, T, env.num_agents, env.obs_dim
        A, D = self.A, self.D
        self.na = na = A if opp_kind is None else A // 2
        nvec, n_shoot, _ = P._action_heads(env.action_space)
        self.nh = len(nvec) + n_shoot
        a = types.SimpleNamespace(hidden_size="128 128", act_hidden_size="128 128", recurrent_hidden_size=128, recurrent_hidden_layers=1,
                                  activation_id=1, use_feature_normalization=True, use_prior=n_shoot > 0, use_recurrent_policy=True,
                                  buffer_size=T, n_rollout_threads=E, gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False)
        cent = env.share_observation_space
        self.policy = P.DeviceMAPPOPolicy(env.observation_space, cent, env.action_space, a, seed=3)
        self.policy.load_state_dict(*state_dicts(D, A * D, nvec, n_shoot, 50))
        self.buffer = pkg.DeviceSharedReplayBuffer(a, na, env.observation_space, cent, env.action_space)
        self.opp = None
        if opp_kind == "pool":
            self.opp = P.DevicePolicyPool(env.observation_space, env.action_space, a, 3, form="mappo", seed=4)
            for k in range(3):
                self.opp.load_state_dict(k, state_dicts(D, A * D, nvec, n_shoot, 60 + k)[0])
            self.opp.assign_split(E, [0, 1, 2], na=A - na)
        elif opp_kind == "policy":
            self.opp = P.DeviceMAPPOPolicy(env.observation_space, cent, env.action_space, a, seed=4, critic=False)
            self.opp.load_state_dict(state_dicts(D, A * D, nvec, n_shoot, 60)[0])
        obs, share = env.reset()
        self.buffer.set_slot("obs", 0, obs[:, :na])
        self.buffer.set_slot("share_obs", 0, share[:, :na])
        self.ro = pkg.DeviceMAPPORollout(env, self.policy, self.buffer, opponent=self.opp, num_learner_agents=na)
        self.h_opp, self.m_opp = self.ro.opponent_states, self.ro.opponent_masks      # both paths keep the opponent's state here
        self.views = {k: self.buffer.device_tensor(k) for k in ("obs", "share_obs", "rnn_states_actor", "rnn_states_critic", "masks")}

    def post_step_bytes(self):
        """(bytes written, bytes read) by one post-step launch when no env is done: the buffer rows out, the env's arrays in (each obs
        block is read na times for share_obs, from L2 after the first)."""
        N, W, D, nh = self.E * self.na, self.A * self.D, self.D, self.nh
        written = 4 * (N * (W + D + 2 * nh + 3) + self.E * (self.A - self.na))
        read = 4 * (N * (W + D + nh + 2)) + self.E * self.A * (1 + self.na)
        return written, read

    def python_loop(self):
        env, pol, buf, na, A, D, nh, E = self.env, self.policy, self.buffer, self.na, self.A, self.D, self.nh, self.E
        act, obs, rew, done, _ = env.device_tensors()
        v = self.views
        cur = torch.cuda.current_stream()
        for s in range(self.T):
            values, actions, logp, ha, hc = pol.get_actions(v["share_obs"][s].reshape(-1, A * D), v["obs"][s].reshape(-1, D),
                                                            v["rnn_states_actor"][s].reshape(-1, 1, 128),
                                                            v["rnn_states_critic"][s].reshape(-1, 1, 128), v["masks"][s].reshape(-1, 1))
            act[:, :na, :nh] = actions.view(E, na, nh)
            if self.opp is not None:
                self.opp.act_into_env(env, self.h_opp, self.m_opp, agents=slice(na, A))
            env.step_device(stream=cur)
            dones = done.reshape(E, A).bool()
            dones_env = dones.all(dim=1)
            keep = (~dones_env).float()
            ha, hc = ha.view(E, na, 128) * keep[:, None, None], hc.view(E, na, 128) * keep[:, None, None]
            masks = keep[:, None, None].expand(E, A, 1)
            active = 1.0 - (dones & ~dones_env[:, None]).float()[:, :, None]
            if self.opp is not None:
                self.h_opp.view(E, A - na, 128).mul_(keep[:, None, None])
                self.m_opp.copy_(masks[:, na:].reshape(-1, 1))
            share = obs.reshape(E, 1, A * D).expand(E, na, A * D)
            ins = [obs[:, :na].contiguous(), share.contiguous(), act[:, :na, :nh].contiguous(), rew[:, :na].contiguous(),
                   masks[:, :na].contiguous(), logp.view(E, na, 1).expand(E, na, nh).contiguous(), values, ha, hc]
            cur.synchronize()            # insert copies on the buffer's own stream
            buf.insert(*ins, active_masks=active[:, :na].contiguous(), on_device=True)

    def collect(self):
        self.ro.collect()

    def timed(self, fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        self.env.sync()
        self.buffer.after_update()
        return wall * 1e6 / self.T, e0.elapsed_time(e1) * 1e3 / self.T

    def close(self):
        for x in (self.ro, self.opp, self.policy, self.buffer, self.env):
            if x is not None:
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
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shape", default=None)
    ap.add_argument("--trace", action="store_true", help="collect only, for a rocprofv3 kernel trace of one shape")
    ap.add_argument("--stats", default=None, help="directory of the kernel traces: <stats>/<shape>/**/*kernel_stats.csv")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mappo_rollout_bench.txt"))
    a = ap.parse_args()
    shapes = [a.shape] if a.shape else list(SHAPES)
    if a.trace:
        for shape in shapes:
            h = Handles(shape, a.envs, a.steps)
            for _ in range(TRACE_ROLLOUTS):
                h.timed(h.collect)
            h.close()
        return
    fmt = lambda x: f"{np.median(x):8.1f} ({min(x):.1f} .. {max(x):.1f})"
    lines = [f"# a MAPPO rollout of {a.steps} steps at {a.envs} envs, the Python loop of INTEGRATION.md 5e vs DeviceMAPPORollout.collect on the same "
             f"handles, {torch.cuda.get_device_name(0)}; {a.reps} rollouts of each, alternating, after one warm-up of each. us per step, median "
             "(min .. max): wall = host clock around the rollout + synchronise; stream = HIP events on torch's stream around it. kernels = the "
             "per-step kernels' own average times, summed, from a rocprofv3 kernel trace of collect ONLY (a run of its own; a kernel counts as "
             "per-step when its calls are a whole multiple of the traced steps). post-step = rollout_share_post_kernel's own average time from "
             f"that trace, the bytes one launch writes and reads (no env done), and their rate against an HBM peak of {HBM_PEAK / 1e12:.0f} TB/s "
             "(the reads of share_obs's sources hit L2 after the first)."]
    for shape in shapes:
        first = len(lines) if shape != shapes[0] else 0
        h = Handles(shape, a.envs, a.steps)
        res = {"python loop": ([], []), "collect": ([], [])}
        for rep in range(a.reps + 1):
            for name, fn in (("python loop", h.python_loop), ("collect", h.collect)):
                w, s = h.timed(fn)
                if rep:
                    res[name][0].append(w)
                    res[name][1].append(s)
        lines.append(f"{shape}: {h.E} envs x {h.A} agents, learner rows {h.E * h.na}, opponent rows {h.E * (h.A - h.na)}, obs {h.D}, "
                     f"share_obs {h.A * h.D}, heads {h.nh}")
        for name, (w, s) in res.items():
            lines.append(f"  {name:>12}  wall {fmt(w)}  stream {fmt(s)}  steps/s {1e6 / np.median(w):9.0f}")
        lines.append(f"  {'speed-up':>12}  wall x{np.median(res['python loop'][0]) / np.median(res['collect'][0]):.2f}")
        wr, rd = h.post_step_bytes()
        if a.stats:
            tot, rows = kernel_sum(a.stats, shape, TRACE_ROLLOUTS * a.steps)
            if tot is None:
                lines.append("  kernels: no trace found")
            else:
                gap = np.median(res["collect"][1]) - tot / 1e3
                lines.append(f"  {'kernels':>12}  {tot / 1e3:8.1f} us per step; collect's stream time leaves {gap:.1f} us per step between them")
                for name, n, avg in rows:
                    lines.append(f"      {n} x {avg / 1e3:7.1f} us  {name[:110]}")
                post = [avg for name, _, avg in rows if POST_KERNEL in name]
                if post:
                    t = post[0] * 1e-9
                    lines.append(f"  {'post-step':>12}  {post[0] / 1e3:7.1f} us; writes {wr / 1e6:.2f} MB, reads {rd / 1e6:.2f} MB: "
                                 f"{wr / t / 1e12:.2f} TB/s written = {100 * wr / t / HBM_PEAK:.0f} % of peak, "
                                 f"{(wr + rd) / t / 1e12:.2f} TB/s moved = {100 * (wr + rd) / t / HBM_PEAK:.0f} %")
        else:
            lines.append(f"  {'post-step':>12}  writes {wr / 1e6:.2f} MB, reads {rd / 1e6:.2f} MB per launch (no trace given: no time)")
        print("\n".join(lines[first:]), flush=True)
        h.close()
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(txt)


if __name__ == "__main__":
    main()
