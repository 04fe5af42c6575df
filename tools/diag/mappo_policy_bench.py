#!/usr/bin/env python3
"""Time DeviceMAPPOPolicy.get_actions (actor + centralised critic) and .get_values at 8192 / 16 384 / 32 768 rows, both arithmetic forms,
for two cases of tests/golden/mappo_*.npz: 2v2 scenario2_nvn (obs 39, cent_obs 156, Tuple heads, use_prior) and 4v4 RWR (obs 65,
cent_obs 520, feature norm). Beside them: an eager torch restatement of the same network and sampler (fp32, one multinomial per
categorical head, Bernoulli munition heads), and DevicePolicy at the same rows as a control against profiles/policy_bench.txt (the same
seeded case as tools/diag/policy_bench.py). Kernel time: events around `reps` back-to-back calls; wall time: host time per call with a
synchronise after each (median). Output: profiles/mappo_policy_bench.txt ("The PPO rollout policy").

    python tools/diag/mappo_policy_bench.py [--reps 200]
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
torch.cuda.init()
import aircombat_selfplay_amd  # noqa: E402,F401
import mappo_util as M  # noqa: E402
import policy_bench as PB  # noqa: E402
import policy_util as U  # noqa: E402

P = importlib.import_module("aircombat-selfplay_amd.policy")


def eager(sd, csd, nvec, n_shoot, fn):
    t = {k: torch.as_tensor(v).cuda() for k, v in sd.items()}
    c = {k: torch.as_tensor(v).cuda() for k, v in csd.items()}

    def mlp(w, p, x):
        for i in (0, 3):
            x = F.layer_norm(F.relu(F.linear(x, w[f"{p}{i}.weight"], w[f"{p}{i}.bias"])), (128,), w[f"{p}{i + 2}.weight"], w[f"{p}{i + 2}.bias"])
        return x

    def trunk(w, x, h, m):
        if fn:
            x = F.layer_norm(x, (x.shape[-1],), w["base.feature_norm.weight"], w["base.feature_norm.bias"])
        x = mlp(w, "base.mlp.fc.", x)
        h = torch._VF.gru_cell(x, h.reshape(-1, 128) * m, w["rnn.gru.weight_ih_l0"], w["rnn.gru.weight_hh_l0"], w["rnn.gru.bias_ih_l0"], w["rnn.gru.bias_hh_l0"])
        return F.layer_norm(h, (128,), w["rnn.norm.weight"], w["rnn.norm.bias"]), h

    def critic(cobs, hc, m):
        y, hc2 = trunk(c, cobs, hc, m)
        return F.linear(mlp(c, "mlp.fc.", y), c["value_out.weight"], c["value_out.bias"]), hc2

    def get_actions(cobs, obs, ha, hc, m):
        x, ha2 = trunk(t, obs, ha, m)
        x = mlp(t, "act.mlp.fc.", x)
        acts, lps = [], []
        for i in range(len(nvec)):
            ls = torch.log_softmax(F.linear(x, t[f"act.action_outs.{i}.logits_net.weight"], t[f"act.action_outs.{i}.logits_net.bias"]), -1)
            a = torch.multinomial(ls.exp(), 1)
            acts.append(a.float())
            lps.append(ls.gather(-1, a))
        if n_shoot:
            ang, dist = torch.rad2deg(obs[:, 11:12]), obs[:, 13:14] * 10000
            a0 = torch.where(dist <= 8000, 10.0, torch.where(dist <= 12000, 6.0, 3.0))
            b0 = torch.where(ang <= 22.5, 3.0, torch.where(ang <= 45, 6.0, 10.0))
            for s in range(n_shoot):
                k = len(nvec) + s
                y = 100 - F.softplus(100 - F.softplus(F.linear(x, t[f"act.action_outs.{k}.net.weight"], t[f"act.action_outs.{k}.net.bias"])))
                p = (1 + y[:, :1] + a0) / (2 + y[:, :1] + y[:, 1:] + a0 + b0)
                d = torch.distributions.Bernoulli(probs=p)
                f = d.sample()
                acts.append(f)
                lps.append(d.log_prob(f))
        v, hc2 = critic(cobs, hc, m)
        return v, torch.cat(acts, -1), torch.cat(lps, -1).sum(-1, keepdim=True), ha2, hc2

    return get_actions, lambda cobs, hc, m: critic(cobs, hc, m)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mappo_policy_bench.txt"))
    a = ap.parse_args()
    lines = [f"# DeviceMAPPOPolicy vs eager torch, {torch.cuda.get_device_name(0)}; {a.reps} calls. us per call: 'stream' = events around "
             "back-to-back calls, 'wall' = host time of one call + synchronize (median). get_actions = actor + critic on cent_obs; "
             "get_values = critic only; 'ppo' = DevicePolicy.get_actions on the seeded case of profiles/policy_bench.txt (control)"]
    lines.append(f"{'case':>10} {'rows':>6} {'form':>6} {'call':>12} {'stream us':>10} {'wall us':>8}")
    cases = {"2v2": "a", "4v4-rwr": "b"}
    for name, tag in cases.items():
        g = M.golden_case(tag)
        obs_dim, cent, _, nvec, n_shoot, fn, _ = M.CASES[tag]
        o_sp, c_sp, act_sp = M.spaces(tag)
        ref_actions, ref_values = eager(g["sd"], g["critic_sd"], nvec, n_shoot, fn)
        for n in (8192, 16384, 32768):
            idx = np.arange(n) % len(g["obs"])
            obs, cobs = torch.as_tensor(g["obs"][idx]).cuda(), torch.as_tensor(g["cent_obs"][idx]).cuda()
            ha, hc = torch.as_tensor(g["rnn_states"][idx]).cuda(), torch.as_tensor(g["rnn_states_critic"][idx]).cuda()
            m = torch.ones(n, 1, device="cuda")
            for prec in ("fast", "fp32"):
                pol = P.DeviceMAPPOPolicy(o_sp, c_sp, act_sp, M.args(tag), precision=prec, seed=1)
                pol.load_state_dict(g["sd"], g["critic_sd"])
                k, w = PB.timeit(lambda: pol.get_actions(cobs, obs, ha, hc, m), a.reps)
                lines.append(f"{name:>10} {n:>6} {prec:>6} {'get_actions':>12} {k:>10.1f} {w:>8.1f}")
                k, w = PB.timeit(lambda: pol.get_values(cobs, hc, m), a.reps)
                lines.append(f"{name:>10} {n:>6} {prec:>6} {'get_values':>12} {k:>10.1f} {w:>8.1f}")
                pol.close()
            with torch.no_grad():
                k, w = PB.timeit(lambda: ref_actions(cobs, obs, ha, hc, m), a.reps)
                lines.append(f"{name:>10} {n:>6} {'torch':>6} {'get_actions':>12} {k:>10.1f} {w:>8.1f}")
                k, w = PB.timeit(lambda: ref_values(cobs, hc, m), a.reps)
                lines.append(f"{name:>10} {n:>6} {'torch':>6} {'get_values':>12} {k:>10.1f} {w:>8.1f}")
    gs = U.golden()
    sd, csd = U.state_dicts(gs, "b")
    obs_space, act_space = U.spaces("b")
    for n in (8192, 16384, 32768):
        rng = np.random.default_rng(n)
        obs = torch.as_tensor(rng.normal(0, 0.5, (n, 15)).astype(np.float32)).cuda()
        ha = torch.as_tensor(rng.normal(0, 0.5, (n, 1, 128)).astype(np.float32)).cuda()
        hc = ha.clone()
        m = torch.ones(n, 1, device="cuda")
        for prec in ("fast", "fp32"):
            pol = P.DevicePolicy(obs_space, act_space, U.args("b"), precision=prec, seed=1)
            pol.load_state_dict(sd, csd)
            k, w = PB.timeit(lambda: pol.get_actions(obs, ha, hc, m), a.reps)
            lines.append(f"{'ppo':>10} {n:>6} {prec:>6} {'get_actions':>12} {k:>10.1f} {w:>8.1f}")
            k, w = PB.timeit(lambda: pol.get_values(obs, hc, m), a.reps)
            lines.append(f"{'ppo':>10} {n:>6} {prec:>6} {'get_values':>12} {k:>10.1f} {w:>8.1f}")
            pol.close()
    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(txt)


if __name__ == "__main__":
    main()
