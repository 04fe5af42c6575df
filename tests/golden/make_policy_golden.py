"""Generate tests/golden/policy_1v1.npz and policy_seeded.npz from the REFERENCE's own PPO actor / critic (runs only where the
reference tree exists).

algorithms/ppo/ppo_actor.py and ppo_critic.py are imported from the reference and evaluated in float64 on the CPU (gymnasium is stubbed
with the space containers the modules test against, as make_golden.py does). Two cases, 256 rows each:

  policy_1v1.npz     the shipped 1v1_actor.pt (Tuple(MultiDiscrete([3, 5, 3]), MultiDiscrete([2, 2, 2, 2])), use_prior, obs_dim 21),
                     actor only; its state_dict is stored (sd/<key>)
  policy_seeded.npz  actor + critic with MultiDiscrete([41, 41, 41, 30]), use_feature_normalization, obs_dim 15, weights from
                     tests/policy_util.seeded_state_dicts (not stored: the tests regenerate them)

Stored: the observations and masks (the GRU-state inputs come from policy_util.hashed_states), and the reference's deterministic outputs:
actions (int8), log-probs (float64), new GRU states (float32), each head's logits (float32), each munition head's p (float64), and for
the seeded case the values (float64) and the critic's new state (float32). Only data is stored; no reference source text.

    python tests/golden/make_policy_golden.py

policy_edges.npz (``python tests/golden/make_policy_golden.py edges`` writes it alone) pins the restatement at every configuration of
tests/policy_edges_util.py's table: the first 32 rows of the reference's PPOActor / PPOCritic in float64 on the table's hashed weights
and inputs, keys ``<entry>/<array>``: actions (uint8: a head may have 160 categories), log_probs, values, shoot_p (float64), logits, rnn_states_out,
rnn_states_critic_out (float32). The wide entries' critic is the reference's PPOCritic on cent_obs. Nothing else is stored: weights
and inputs come from the hash.
"""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("AC_REFERENCE_ROOT", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import policy_util as U  # noqa: E402
N = 256


def stub_gymnasium():
    g = types.ModuleType("gymnasium")
    sp = types.ModuleType("gymnasium.spaces")

    class Box:
        def __init__(self, low=None, high=None, shape=None, dtype=None):
            self.low, self.high, self.shape = np.full(shape, low), np.full(shape, high), tuple(shape)

    class Discrete:
        def __init__(self, n):
            self.n = n

    class MultiDiscrete:
        def __init__(self, nvec):
            self.nvec = np.array(nvec)
            self.shape = self.nvec.shape

    class MultiBinary:
        def __init__(self, n):
            self.n, self.shape = n, (n,)

    class Dict:
        pass

    class Tuple(tuple):
        def __new__(cls, xs):
            return tuple.__new__(cls, xs)

    sp.Box, sp.Discrete, sp.MultiDiscrete, sp.MultiBinary, sp.Tuple, sp.Dict, sp.Space = Box, Discrete, MultiDiscrete, MultiBinary, Tuple, Dict, object
    g.spaces, g.Space = sp, object
    sys.modules.update({"gymnasium": g, "gymnasium.spaces": sp})
    sys.path.insert(0, REF)
    if not hasattr(np, "product"):   # flatten.py calls np.product, removed in numpy 2
        np.product = np.prod
    return sp


def args_ns(**kw):
    a = types.SimpleNamespace(gain=0.01, hidden_size="128 128", act_hidden_size="128 128", activation_id=1, use_feature_normalization=False,
                              use_recurrent_policy=True, recurrent_hidden_size=128, recurrent_hidden_layers=1, use_prior=False)
    a.__dict__.update(kw)
    return a


def inputs(rng, obs_dim):
    obs = rng.normal(0.0, 0.5, size=(N, obs_dim))
    if obs_dim > 13:   # straddle the prior's thresholds: 22.5 / 45 degrees, 8000 / 12000 m (never closer than 1e-3 to one)
        deg = rng.choice([22.5, 45.0], size=N) + rng.uniform(-3.0, 3.0, size=N)
        deg[N // 2:] = rng.uniform(0.0, 90.0, size=N - N // 2)
        dist = rng.choice([8000.0, 12000.0], size=N) + rng.uniform(-600.0, 600.0, size=N)
        dist[3 * N // 4:] = rng.uniform(2000.0, 20000.0, size=N - 3 * N // 4)
        for th, v in ((22.5, deg), (45.0, deg), (8000.0, dist), (12000.0, dist)):
            near = np.abs(v - th) < 1e-2 * (1 if th < 100 else 100)
            v[near] += 0.05 * (1 if th < 100 else 100)
        obs[:, 11] = np.deg2rad(deg)
        obs[:, 13] = dist / 10000.0
    obs = obs.astype(np.float32)
    masks = (rng.uniform(size=(N, 1)) > 0.25).astype(np.uint8)
    return obs, masks


def head_details(actor, obs64, rnn64, masks64, n_cat, n_shoot):
    """Each head's logits / probabilities and each munition head's p, from the reference's own submodules."""
    with torch.no_grad():
        x = actor.base(obs64)
        x, _ = actor.rnn(x, rnn64, masks64)
        x = actor.act.mlp(x)
        logits = [actor.act.action_outs[i].logits_net(x) for i in range(n_cat)]
        out = {"logits": torch.cat(logits, -1).numpy(), "probs": torch.cat([torch.softmax(l, -1) for l in logits], -1).numpy()}
        if n_shoot:
            ang = torch.rad2deg(obs64[:, 11])
            dist = obs64[:, 13] * 10000
            a0 = torch.full((obs64.shape[0], 1), 3.0, dtype=torch.float64)
            b0 = torch.full((obs64.shape[0], 1), 10.0, dtype=torch.float64)
            a0[dist <= 12000] = 6
            a0[dist <= 8000] = 10
            b0[ang <= 45] = 6
            b0[ang <= 22.5] = 3
            ps = [actor.act.action_outs[n_cat + s](x, alpha0=a0, beta0=b0).probs for s in range(n_shoot)]
            out["shoot_p"] = torch.cat(ps, -1).numpy()
    return out


def main():
    sp = stub_gymnasium()
    from algorithms.ppo.ppo_actor import PPOActor
    from algorithms.ppo.ppo_critic import PPOCritic

    rng = np.random.default_rng(20261015)
    for tag in ("a", "b"):
        obs_dim, nvec, n_shoot, fn, prior, has_c = U.CASES[tag]
        space = sp.MultiDiscrete(nvec)
        act_space = sp.Tuple([space, sp.MultiDiscrete([2] * n_shoot)]) if n_shoot else space
        args = args_ns(use_prior=prior, use_feature_normalization=fn)
        obs_space = sp.Box(low=-10, high=10.0, shape=(obs_dim,))
        actor = PPOActor(args, obs_space, act_space)
        data = {}
        if tag == "a":
            sd = torch.load(os.path.join(REF, "checkpoint", "1v1_actor.pt"), map_location="cpu")
            for k, v in sd.items():
                data[f"sd/{k}"] = v.numpy().astype(np.float32)
            crit = None
        else:
            asd, csd = U.seeded_state_dicts(obs_dim, nvec, fn)
            sd = {k: torch.from_numpy(v) for k, v in asd.items()}
            crit = PPOCritic(args, obs_space)
            crit.load_state_dict({k: torch.from_numpy(v) for k, v in csd.items()})
        actor.load_state_dict(sd)
        obs, masks = inputs(rng, obs_dim)
        rnn = U.hashed_states(U.SEED_RNN, N)
        data["obs"], data["masks"] = obs, masks
        actor.double()
        actor.tpdv = dict(dtype=torch.float64, device=torch.device("cpu"))
        obs64, rnn64, m64 = (torch.from_numpy(x.astype(np.float64)) for x in (obs, rnn, masks))
        with torch.no_grad():
            act, logp, h = actor(obs64, rnn64, m64, deterministic=True)
        data["actions"], data["log_probs"], data["rnn_states_out"] = act.numpy().astype(np.int8), logp.numpy(), h.numpy().astype(np.float32)
        det = head_details(actor, obs64, rnn64, m64, len(nvec), n_shoot)
        data["logits"] = det["logits"].astype(np.float32)
        if n_shoot:
            data["shoot_p"] = det["shoot_p"]
        if crit is not None:
            crit.double()
            crit.tpdv = dict(dtype=torch.float64, device=torch.device("cpu"))
            with torch.no_grad():
                val, hc = crit(obs64, torch.from_numpy(U.hashed_states(U.SEED_RNN_CRITIC, N).astype(np.float64)), m64)
            data["values"], data["rnn_states_critic_out"] = val.numpy(), hc.numpy().astype(np.float32)
        out = os.path.join(HERE, U.FILES[tag])
        np.savez_compressed(out, **data)
        print(f"wrote {out}: {len(data)} arrays, {os.path.getsize(out)} bytes")


def edges():
    sp = stub_gymnasium()
    from algorithms.ppo.ppo_actor import PPOActor
    from algorithms.ppo.ppo_critic import PPOCritic
    import policy_edges_util as E

    data, R = {}, E.GOLDEN_ROWS
    for name, e in E.ENTRIES.items():
        d = E.inputs(name)
        space = sp.MultiDiscrete(e.nvec)
        act_space = sp.Tuple([space, sp.MultiDiscrete([2] * e.n_shoot)]) if e.n_shoot else space
        args = args_ns(use_prior=e.n_shoot > 0, use_feature_normalization=e.fn)
        actor = PPOActor(args, sp.Box(low=-10, high=10.0, shape=(e.obs_dim,)), act_space)
        actor.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in d["sd"].items()})
        crit = PPOCritic(args, sp.Box(low=-10, high=10.0, shape=(E.critic_dim(e),)))
        crit.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in d["critic_sd"].items()})
        for m in (actor, crit):
            m.double()
            m.tpdv = dict(dtype=torch.float64, device=torch.device("cpu"))
        t64 = lambda x: torch.from_numpy(np.asarray(x[:R], dtype=np.float64))
        obs64, m64 = t64(d["obs"]), t64(d["masks"])
        with torch.no_grad():
            act, logp, h = actor(obs64, t64(d["rnn_states"]), m64, deterministic=True)
            val, hc = crit(t64(E.critic_input(e, d)), t64(d["rnn_states_critic"]), m64)
        det = head_details(actor, obs64, t64(d["rnn_states"]), m64, len(e.nvec), e.n_shoot)
        data[f"{name}/actions"], data[f"{name}/log_probs"], data[f"{name}/values"] = act.numpy().astype(np.uint8), logp.numpy(), val.numpy()
        data[f"{name}/logits"] = det["logits"].astype(np.float32)
        data[f"{name}/rnn_states_out"], data[f"{name}/rnn_states_critic_out"] = h.numpy().astype(np.float32), hc.numpy().astype(np.float32)
        if e.n_shoot:
            data[f"{name}/shoot_p"] = det["shoot_p"]
    np.savez_compressed(E.GOLDEN, **data)
    print(f"wrote {E.GOLDEN}: {len(data)} arrays, {os.path.getsize(E.GOLDEN)} bytes")


if __name__ == "__main__":
    if sys.argv[1:] != ["edges"]:
        main()
    edges()
