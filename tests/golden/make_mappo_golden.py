"""Generate tests/golden/mappo_{a,b,c,d}.npz from the REFERENCE's own MAPPO actor / critic (runs only where the reference tree exists).

algorithms/mappo/ppo_actor.py and ppo_critic.py are imported from the reference and evaluated in float64 on the CPU, with gymnasium
stubbed as make_policy_golden.py does. Four cases of 256 rows (tests/mappo_util.CASES), the observations grouped by env [E, A, obs_dim]
so that cent_obs (each env's observations concatenated, the critic's input) is derived, not stored:

  a  scenario2_nvn:     obs 39, cent 156, Tuple(MultiDiscrete([3, 5, 3]), MultiDiscrete([2, 2, 2, 2])), use_prior
  b  4v4 RWR:           obs 65, cent 520, the same heads, use_feature_normalization
  c  MultipleCombat 4v4: obs 51, cent 408, MultiDiscrete([41, 41, 41, 30])
  d  legacy 4v4:        the shipped 4v4_actor.pt (obs 21, the Tuple heads, use_prior; its state_dict stored as sd/<key>), cent 168

Weights (all but d's actor) and GRU-state inputs come from the exact integer hash of tests/policy_util.py and are not stored. Stored:
obs, masks, and the reference's deterministic outputs: actions (int8), log-probs (float64), new GRU states (float32), logits (float32),
munition p (float64), values (float64), the critic's new state (float32). Only data is stored; no reference source text.

    python tests/golden/make_mappo_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_policy_golden as MP  # noqa: E402
import mappo_util as M  # noqa: E402
import policy_util as U  # noqa: E402


def main():
    sp = MP.stub_gymnasium()
    from algorithms.mappo.ppo_actor import PPOActor
    from algorithms.mappo.ppo_critic import PPOCritic

    rng = np.random.default_rng(20261016)
    for tag in ("a", "b", "c", "d"):
        obs_dim, cent, A, nvec, n_shoot, fn, prior = M.CASES[tag]
        space = sp.MultiDiscrete(nvec)
        act_space = sp.Tuple([space, sp.MultiDiscrete([2] * n_shoot)]) if n_shoot else space
        args = MP.args_ns(use_prior=prior, use_feature_normalization=fn)
        actor = PPOActor(args, sp.Box(low=-10, high=10.0, shape=(obs_dim,)), act_space)
        critic = PPOCritic(args, sp.Box(low=-10, high=10.0, shape=(cent,)))
        asd, csd = M.seeded_state_dicts(tag)
        data = {}
        if asd is None:
            sd = torch.load(os.path.join(MP.REF, "checkpoint", "4v4_actor.pt"), map_location="cpu")
            for k, v in sd.items():
                data[f"sd/{k}"] = v.numpy().astype(np.float32)
        else:
            sd = {k: torch.from_numpy(v) for k, v in asd.items()}
        actor.load_state_dict(sd)
        critic.load_state_dict({k: torch.from_numpy(v) for k, v in csd.items()})
        obs, masks = MP.inputs(rng, obs_dim)
        E = MP.N // A
        data["obs"], data["masks"] = obs.reshape(E, A, obs_dim), masks
        cobs = M.cent_obs(data["obs"])
        for net in (actor, critic):
            net.double()
            net.tpdv = dict(dtype=torch.float64, device=torch.device("cpu"))
        rnn = U.hashed_states(U.SEED_RNN, MP.N)
        obs64, cobs64, rnn64, m64 = (torch.from_numpy(x.astype(np.float64)) for x in (obs, cobs, rnn, masks))
        with torch.no_grad():
            act, logp, h = actor(obs64, rnn64, m64, deterministic=True)
            val, hc = critic(cobs64, torch.from_numpy(U.hashed_states(U.SEED_RNN_CRITIC, MP.N).astype(np.float64)), m64)
        data["actions"], data["log_probs"], data["rnn_states_out"] = act.numpy().astype(np.int8), logp.numpy(), h.numpy().astype(np.float32)
        det = MP.head_details(actor, obs64, rnn64, m64, len(nvec), n_shoot)
        data["logits"] = det["logits"].astype(np.float32)
        if n_shoot:
            data["shoot_p"] = det["shoot_p"]
        data["values"], data["rnn_states_critic_out"] = val.numpy(), hc.numpy().astype(np.float32)
        out = os.path.join(HERE, M.FILES[tag])
        np.savez_compressed(out, **data)
        print(f"wrote {out}: {len(data)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
