#!/usr/bin/env python3
"""Mutual-support discriminator timings on one MI355X -> profiles/mutual_support_bench.txt ("The
mutual-support scorer").

For 4096 envs x 64 steps, 2v2 (obs 39, 7 action columns, 2 agents) and 4v4 RWR (obs 65, 4 agents), on a DeviceSharedReplayBuffer with
random contents:
  intrinsic_rewards   DeviceDiscriminator.intrinsic_rewards(buffer, add=False) against an eager-torch restatement on the same device
                      tensors: the gather by indexing the buffer's views, cat, the Linears, the squared errors and their difference
  scorer launch       ac_mi_score alone (HIP events around back-to-back launches), with the fp32 operations the two nets need for the
                      2 n E tuples (2 x in x out per Linear, padding not counted) over that time, against the 157 TFLOP/s fp32 matrix peak
  train               DeviceDiscriminator.train(buffer) (one epoch of --minibatches mini-batches) against the same steps in eager torch:
                      indexing and cat for the gather, the same Linears and losses, torch's Adam
The members of a comparison alternate call by call. Each is the median HIP-event time over back-to-back calls and the median wall time
per call with a synchronise, after warm-up; train ends with a host read, so its wall time is the figure.

    python tools/diag/mutual_support_bench.py [--reps 10] [--envs 4096] [--steps 64] [--out profiles/mutual_support_bench.txt]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import aircombat_selfplay_amd as pkg  # noqa: E402

CASES = [("2v2", 2, 39, 7), ("4v4 RWR", 4, 65, 7)]      # name, learner agents, obs_dim, action columns
PEAK = 157e12


class Space:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def timed(fns, reps, warm=2):
    """[(device ms, wall ms)] per function, the functions alternating call by call."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)] for _ in range(reps)]
    for e in ev:
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mutual_support_bench.txt"))
    a = ap.parse_args()
    E, T = a.envs, a.steps
    torch.manual_seed(0)
    lines = [f"# tools/diag/mutual_support_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {E} envs x {T} steps, median of "
             f"{a.reps} (ms): device = HIP events over back-to-back calls, wall = per call with a synchronise"]
    try:
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        lines.append(f"# parent commit {rev or '?'} plus the working tree of this change")
    except OSError:
        pass
    lines.append(f"{'case':8s} {'what':58s} {'device':>9} {'wall':>9}")

    def row(case, what, r, tail=""):
        lines.append(f"{case:8s} {what:58s} {r[0]:9.3f} {r[1]:9.3f}{tail}")
        print(lines[-1], flush=True)

    lib = pkg.load_library()
    for case, na, D, Cc in CASES:
        bargs = types.SimpleNamespace(buffer_size=T, n_rollout_threads=E, gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False,
                                      recurrent_hidden_size=128, recurrent_hidden_layers=1)
        buf = pkg.DeviceSharedReplayBuffer(bargs, na, D, na * D, Space(shape=(Cc,), nvec=np.full(Cc, 41)))
        obs, act, rnn = buf.device_tensor("obs"), buf.device_tensor("actions"), buf.device_tensor("rnn_states_actor")
        obs.normal_()
        rnn.uniform_(-1.0, 1.0)
        act.copy_(torch.randint(0, 41, act.shape, device="cuda").float())
        dargs = types.SimpleNamespace(ppo_epoch=1, num_mini_batch=a.minibatches, hidden_size="128 128", recurrent_hidden_size=128, lr=5e-4,
                                      data_chunk_length=8, intrinsic_ratio=0.1)
        parts = Space(spaces=(Space(nvec=np.full(Cc - Cc // 2, 41)), Space(nvec=np.full(Cc // 2, 2))))
        disc = pkg.DeviceDiscriminator(dargs, na, Space(shape=(D,)), Space(shape=(na * D,)), parts, device=torch.device("cuda", 0))
        h_all, K1 = rnn[:, :, 0, 0, :], 128 + 2 * Cc

        def tuples(times):
            X, Y = [], []
            for j in (0, 1):
                X.append(torch.cat([h_all[times], act[times][:, :, j], act[times][:, :, 1 - j]], -1).reshape(-1, K1))
                Y.append(obs[times + 1][:, :, j].reshape(-1, D))
            return torch.cat(X), torch.cat(Y)

        all_steps = torch.arange(T, device="cuda")

        @torch.no_grad()
        def eager_rewards():
            X, Y = tuples(all_steps)
            with_act = ((disc.pred(X) - Y) ** 2).mean(-1)
            without = ((disc.pred_wo(X[:, :128 + Cc]) - Y) ** 2).mean(-1)
            sc = (without - with_act).reshape(2, T, E)
            out = torch.zeros(T, E, na, 1, device="cuda")
            out[:, :, 0, 0], out[:, :, 1, 0] = sc[1], sc[0]
            return out

        fused_rewards = lambda: disc.intrinsic_rewards(buf, add=False)
        ref, got = eager_rewards(), fused_rewards()
        torch.cuda.synchronize()
        diff = float((ref - got).abs().max())
        r = timed([fused_rewards, eager_rewards], a.reps)
        row(case, "intrinsic_rewards: fused scorer (one launch)", r[0], f"   max|fused - eager| {diff:.2e}")
        row(case, "intrinsic_rewards: eager torch (index, cat, Linears, mse)", r[1])

        score_args = disc._score_args(buf, 0, T, 0.0, False, got.data_ptr() if na == 2 else torch.empty(T, E, 2, device="cuda").data_ptr(), None)
        stream = torch.cuda.current_stream().cuda_stream

        def launch():
            assert lib.ac_mi_score(C.byref(score_args), stream) == 0, lib.last_error()

        k = timed([launch], a.reps)[0]
        rows = 2 * T * E
        flop = rows * 2.0 * sum(i * o for i, o in ((K1, 256), (256, 256), (256, D), (128 + Cc, 256), (256, 256), (256, D)))
        row(case, "scorer launch alone (ac_mi_score)", k, f"   {flop / 1e9:.1f} GFLOP, {flop / (k[0] * 1e-3) / 1e12:.1f} TFLOP/s fp32 = "
                                                        f"{100 * flop / (k[0] * 1e-3) / PEAK:.1f} % of the 157 TFLOP/s matrix peak")

        # ---- training: the same steps both ways, each on its own copy of the weights
        eager = pkg.DeviceDiscriminator(dargs, na, Space(shape=(D,)), Space(shape=(na * D,)), parts, device=torch.device("cuda", 0))
        eager.load_state_dict(disc.state_dict())
        mb = T // a.minibatches

        def eager_train():
            order = torch.randperm(T, device="cuda")
            losses = torch.zeros(a.minibatches, device="cuda")
            for i in range(a.minibatches):
                X, Y = tuples(order[i * mb:(i + 1) * mb])
                loss = eager.minibatch_loss(X, Y)
                eager.q_optimizer.zero_grad()
                loss.backward()
                eager.q_optimizer.step()
                losses[i] = loss.detach()
            return float(losses.mean())

        r = timed([lambda: disc.train(buf), eager_train], max(3, a.reps // 2), warm=1)
        row(case, f"train, 1 epoch x {a.minibatches} mini-batches: gather launch + device Adam", r[0])
        row(case, f"train, 1 epoch x {a.minibatches} mini-batches: eager torch", r[1])
        del disc, eager, obs, act, rnn, h_all, buf
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
