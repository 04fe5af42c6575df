#!/usr/bin/env python3
"""Time one DevicePolicyPool.act_into_env against the two ways of acting for K self-play opponents it replaces: K separate
DevicePolicy calls over the reference's np.array_split env ranges, and the reference-style eager torch loop (one actor forward with
sampling per opponent on its env range). The 1v1 PPO form (singlecombat: obs 15, MultiDiscrete([41, 41, 41, 30]), feature norm; the
opponents on agent 1) at 4096 and 16 384 envs with K = 1, 2, 4, 8, 16, both tile orders of the pool; the cost of assign; and the MAPPO
form at one NvN size (scenario2_nvn 2v2, 4096 envs, the opponents on agents 2-3). Times are us per step: 'stream' = events around
back-to-back calls, 'wall' = host time of one call + synchronize (median). Output: profiles/policy_pool_bench.txt ("The
opponent pool").

    python tools/diag/policy_pool_bench.py [--reps 200]
"""
import argparse
import importlib
import os
import sys
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
torch.cuda.init()
import aircombat_selfplay_amd as pkg  # noqa: E402
import policy_util as U  # noqa: E402

P = importlib.import_module("aircombat-selfplay_amd.policy")


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
    for _ in range(max(reps // 4, 5)):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    return kern, float(np.median(walls)) * 1e6


def args(fn, prior):
    return types.SimpleNamespace(hidden_size="128 128", act_hidden_size="128 128", recurrent_hidden_size=128, recurrent_hidden_layers=1,
                                 activation_id=1, use_feature_normalization=fn, use_prior=prior, use_recurrent_policy=True)


def member_sd(obs_dim, nvec, n_shoot, fn, seed):
    a = U.seeded_state_dicts(obs_dim, nvec, fn, seed=seed)[0]
    for s in range(n_shoot):
        k = len(nvec) + s
        a[f"act.action_outs.{k}.net.weight"] = (U.hashed(seed * 1000 + 300 + s, 256) / np.sqrt(128)).reshape(2, 128).astype(np.float32)
        a[f"act.action_outs.{k}.net.bias"] = (U.hashed(seed * 1000 + 400 + s, 2) / np.sqrt(128)).astype(np.float32)
    return a


def eager_actor(sd, nvec, fn):
    """The reference's actor forward with sampling (MultiDiscrete heads), fp32 torch ops, for one opponent's rows."""
    t = {k: torch.as_tensor(v).cuda() for k, v in sd.items()}

    def mlp(p, x):
        for i in (0, 3):
            x = F.layer_norm(F.relu(F.linear(x, t[f"{p}{i}.weight"], t[f"{p}{i}.bias"])), (128,), t[f"{p}{i + 2}.weight"], t[f"{p}{i + 2}.bias"])
        return x

    def act(obs, h, m):
        x = F.layer_norm(obs, (obs.shape[-1],), t["base.feature_norm.weight"], t["base.feature_norm.bias"]) if fn else obs
        x = mlp("base.mlp.fc.", x)
        h = torch._VF.gru_cell(x, h.reshape(-1, 128) * m, t["rnn.gru.weight_ih_l0"], t["rnn.gru.weight_hh_l0"], t["rnn.gru.bias_ih_l0"],
                               t["rnn.gru.bias_hh_l0"])
        x = mlp("act.mlp.fc.", F.layer_norm(h, (128,), t["rnn.norm.weight"], t["rnn.norm.bias"]))
        acts = [torch.multinomial(torch.softmax(F.linear(x, t[f"act.action_outs.{i}.logits_net.weight"],
                                                         t[f"act.action_outs.{i}.logits_net.bias"]), -1), 1) for i in range(len(nvec))]
        return torch.cat(acts, -1).float(), h

    return act


def split(E, K):
    return [(int(r[0]), int(r[-1]) + 1) for r in np.array_split(np.arange(E), K)]


def bench_form(form, E, Ks, reps, lines, eager=True):
    cfg = pkg.default_config("singlecombat" if form == "ppo" else "scenario2_nvn")
    env = (pkg.HipVecEnv if form == "ppo" else pkg.HipShareVecEnv)(cfg, E, device_id=0, seed=1)
    env.reset()
    A, D = env.num_agents, env.obs_dim
    a0, a1 = A // 2, A
    na = a1 - a0
    nvec, n_shoot, _ = P._action_heads(env.action_space)
    fn, prior = form == "ppo", n_shoot > 0
    act_d, obs_d, _, _, _ = env.device_tensors()
    n = E * na
    rng = np.random.default_rng(E)
    h = torch.as_tensor(rng.normal(0, 0.5, (n, 1, 128)).astype(np.float32)).cuda()
    m = torch.ones(n, 1, device="cuda")
    ho = torch.empty_like(h)
    lp = torch.empty(n, 1, device="cuda")
    Kmax = max(Ks)
    sds = [member_sd(D, nvec, n_shoot, fn, 50 + k) for k in range(Kmax)]
    pool = P.DevicePolicyPool(env.observation_space, env.action_space, args(fn, prior), Kmax, form=form, seed=3)
    for k, sd in enumerate(sds):
        pool.load_state_dict(k, sd)
    if form == "ppo":
        singles = [P.DevicePolicy(env.observation_space, env.action_space, args(fn, prior), seed=3, critic=False) for _ in range(Kmax)]
    else:
        cent = pkg.vec_env._Box(-10, 10, (A * D,))
        singles = [P.DeviceMAPPOPolicy(env.observation_space, cent, env.action_space, args(fn, prior), seed=3, critic=False) for _ in range(Kmax)]
    for p, sd in zip(singles, sds):
        p.load_state_dict(sd)
    eagers = [eager_actor(sd, nvec, fn) for sd in sds] if eager else None
    for K in Ks:
        members = np.empty(E, np.int32)
        for k, (e0, e1) in enumerate(split(E, K)):
            members[e0:e1] = k
        t_assign, w_assign = timeit(lambda: pool.assign(members, check=False, na=na), reps // 4)
        _, w_check = timeit(lambda: pool.assign(members, check=True, na=na), reps // 8)
        res = {}
        for xcd in (False, True):
            pool.set_tile_order(xcd)
            res["pool-xcd" if xcd else "pool"] = timeit(lambda: pool.act_into_env(env, h, m, agents=slice(a0, a1), rnn_states_out=ho, logp_out=lp), reps)
        pool.set_tile_order(True)   # the default
        rng_k = split(E, K)

        def sep():
            for k, (e0, e1) in enumerate(rng_k):
                rows = P.AcPolicyRows((e1 - e0) * na, na, A, a0, env.act_dim)
                singles[k]._launch(rows, obs_d[e0:e1], h[e0 * na:e1 * na], None, m[e0 * na:e1 * na], False, None, act_d[e0:e1],
                                   lp[e0 * na:e1 * na], ho[e0 * na:e1 * na], None, None)
        res[f"{K} calls"] = timeit(sep, reps)
        if eager:
            def loop():
                with torch.no_grad():
                    for k, (e0, e1) in enumerate(rng_k):
                        a, hk = eagers[k](obs_d[e0:e1, a0:a1].reshape(-1, D), h[e0 * na:e1 * na], m[e0 * na:e1 * na])
                        act_d[e0:e1, a0:a1, :len(nvec)] = a.reshape(e1 - e0, na, -1)
                        ho[e0 * na:e1 * na] = hk.reshape(-1, 1, 128)
            res["eager torch"] = timeit(loop, max(reps // 4, 10))
        for name, (k_us, w_us) in res.items():
            lines.append(f"{form:>6} {E:>6} {n:>6} {K:>3} {name:>12} {k_us:>10.1f} {w_us:>8.1f}")
        lines.append(f"{form:>6} {E:>6} {n:>6} {K:>3} {'assign':>12} {t_assign:>10.1f} {w_assign:>8.1f}   (check=True wall {w_check:.1f}; "
                     f"{pool.num_tiles} tiles)")
        print("\n".join(lines[-len(res) - 1:]), flush=True)
    for p in singles + [pool]:
        p.close()
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_pool_bench.txt"))
    a = ap.parse_args()
    lines = [f"# DevicePolicyPool.act_into_env vs K DevicePolicy calls over np.array_split env ranges vs the eager torch loop, "
             f"{torch.cuda.get_device_name(0)}; fast form; {a.reps} calls. us per step: 'stream' = events around back-to-back calls, "
             "'wall' = host time of one call + synchronize (median). pool = member-major tiles, pool-xcd = a member's tiles on one XCD. "
             "assign: check=False (stream / wall), check=True wall",
             f"{'form':>6} {'envs':>6} {'rows':>6} {'K':>3} {'how':>12} {'stream us':>10} {'wall us':>8}"]
    for E in (4096, 16384):
        bench_form("ppo", E, (1, 2, 4, 8, 16), a.reps, lines)
    bench_form("mappo", 4096, (1, 8), a.reps, lines, eager=False)
    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(txt)


if __name__ == "__main__":
    main()
