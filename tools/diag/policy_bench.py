#!/usr/bin/env python3
"""Time DevicePolicy.get_actions (actor + critic, MultiDiscrete([41, 41, 41, 30]), feature norm: the seeded case of
tests/golden/policy_seeded.npz) at 8192 / 16 384 / 32 768 rows in both arithmetic forms, and an eager torch restatement of the same network
and sampler (fp32, Categorical sampling per head) on the same GPU. Kernel time: events around `reps` back-to-back calls; wall time: host
time per call with a synchronise after each. Output: profiles/policy_bench.txt ("The PPO rollout policy").

    python tools/diag/policy_bench.py [--reps 200]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
torch.cuda.init()
import aircombat_selfplay_amd  # noqa: E402,F401
import importlib  # noqa: E402
import policy_util as U  # noqa: E402

P = importlib.import_module("aircombat-selfplay_amd.policy")


def eager(sd, csd, nvec):
    t = {k: torch.as_tensor(v).cuda() for k, v in sd.items()}
    c = {k: torch.as_tensor(v).cuda() for k, v in csd.items()}

    def mlp(w, p, x):
        for i in (0, 3):
            x = F.layer_norm(F.relu(F.linear(x, w[f"{p}{i}.weight"], w[f"{p}{i}.bias"])), (128,), w[f"{p}{i + 2}.weight"], w[f"{p}{i + 2}.bias"])
        return x

    def trunk(w, obs, h, m):
        x = F.layer_norm(obs, (obs.shape[-1],), w["base.feature_norm.weight"], w["base.feature_norm.bias"])
        x = mlp(w, "base.mlp.fc.", x)
        h = torch._VF.gru_cell(x, h.reshape(-1, 128) * m, w["rnn.gru.weight_ih_l0"], w["rnn.gru.weight_hh_l0"], w["rnn.gru.bias_ih_l0"], w["rnn.gru.bias_hh_l0"])
        return F.layer_norm(h, (128,), w["rnn.norm.weight"], w["rnn.norm.bias"]), h

    def get_actions(obs, ha, hc, m):
        x, ha2 = trunk(t, obs, ha, m)
        x = mlp(t, "act.mlp.fc.", x)
        acts, lps = [], []
        for i in range(len(nvec)):
            lg = F.linear(x, t[f"act.action_outs.{i}.logits_net.weight"], t[f"act.action_outs.{i}.logits_net.bias"])
            ls = torch.log_softmax(lg, -1)
            a = torch.multinomial(ls.exp(), 1)
            acts.append(a)
            lps.append(ls.gather(-1, a))
        y, hc2 = trunk(c, obs, hc, m)
        v = F.linear(mlp(c, "mlp.fc.", y), c["value_out.weight"], c["value_out.bias"])
        return v, torch.cat(acts, -1).float(), torch.cat(lps, -1).sum(-1, keepdim=True), ha2, hc2

    return get_actions


def timeit(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    kern = e0.elapsed_time(e1) * 1e3 / reps
    walls = []
    for _ in range(reps // 4):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    return kern, float(np.median(walls)) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_bench.txt"))
    a = ap.parse_args()
    g = U.golden()
    sd, csd = U.state_dicts(g, "b")
    obs_space, act_space = U.spaces("b")
    lines = [f"# DevicePolicy.get_actions vs eager torch, {torch.cuda.get_device_name(0)}; MultiDiscrete([41,41,41,30]) actor + critic, "
             f"obs_dim 15, feature norm; {a.reps} calls. us per call: 'stream' = events around back-to-back calls, 'wall' = host time of "
             "one call + synchronize (median)"]
    lines.append(f"{'rows':>6} {'form':>6} {'stream us':>10} {'wall us':>8}")
    ref = eager(sd, csd, U.CASES["b"][1])
    for n in (8192, 16384, 32768):
        rng = np.random.default_rng(n)
        obs = torch.as_tensor(rng.normal(0, 0.5, (n, 15)).astype(np.float32)).cuda()
        ha = torch.as_tensor(rng.normal(0, 0.5, (n, 1, 128)).astype(np.float32)).cuda()
        hc = ha.clone()
        m = torch.ones(n, 1, device="cuda")
        for prec in ("fast", "fp32"):
            pol = P.DevicePolicy(obs_space, act_space, U.args("b"), precision=prec, seed=1)
            pol.load_state_dict(sd, csd)
            k, w = timeit(lambda: pol.get_actions(obs, ha, hc, m), a.reps)
            lines.append(f"{n:>6} {prec:>6} {k:>10.1f} {w:>8.1f}")
            pol.close()
        with torch.no_grad():
            k, w = timeit(lambda: ref(obs, ha, hc, m), a.reps)
        lines.append(f"{n:>6} {'torch':>6} {k:>10.1f} {w:>8.1f}")
    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(txt)


if __name__ == "__main__":
    main()
