"""Writes tests/golden/ppo_update.npz from the reference's own PPOTrainer.ppo_update (algorithms/ppo/ppo_trainer.py and
algorithms/mappo/ppo_trainer.py) in float64 on the CPU, ``tpdv`` set to float64: three consecutive updates of the stub policy of
tests/ppo_update_util.py (a real torch.optim.Adam over {actor}, {critic}) on that module's hashed samples. Stored per algorithm and
update (``<algo>/<step>/<key>``): the six returned values (``ratio`` as its mean) and, after the update, the four parameters with their
exp_avg and exp_avg_sq. The inputs are not stored: the tests regenerate them. Only data is stored; no reference source text. The
reference's modules import gymnasium, which is stubbed as in make_act_train_golden.py. Before anything is written the actor's gradient
norm is checked to stay below max_grad_norm and the critic's above it, in every update.

    AC_REFERENCE_ROOT=<reference checkout> python tests/golden/make_ppo_update_golden.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ["AC_REFERENCE_ROOT"]
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)
import ppo_update_util as U  # noqa: E402

if "gymnasium" not in sys.modules:
    g, sp = types.ModuleType("gymnasium"), types.ModuleType("gymnasium.spaces")
    for n in ("Box", "Discrete", "MultiDiscrete", "MultiBinary", "Dict", "Space"):
        setattr(sp, n, type(n, (), {}))
    sp.Tuple = type("Tuple", (tuple,), {})
    g.spaces, g.Space = sp, sp.Space
    sys.modules.update({"gymnasium": g, "gymnasium.spaces": sp})


def main():
    out = {}
    for algo in ("ppo", "mappo"):
        trainer = importlib.import_module(f"algorithms.{algo}.ppo_trainer").PPOTrainer(U.trainer_args(), torch.device("cpu"))
        trainer.tpdv = dict(dtype=torch.float64, device=torch.device("cpu"))
        policy = U.StubPolicy(torch.float64)
        for step in range(U.STUB_STEPS):
            ret = trainer.ppo_update(policy, U.stub_sample(step, algo == "mappo"))
            vals = dict(zip(U.RETURNED, ret))
            vals["ratio"] = vals["ratio"].mean()
            assert vals["actor_grad_norm"] < U.ARGS["max_grad_norm"] < vals["critic_grad_norm"], vals
            for k, v in vals.items():
                out[f"{algo}/{step}/{k}"] = np.float64(float(v))
            for name, p in policy.params().items():
                st = policy.optimizer.state[p]
                assert float(st["step"]) == step + 1
                out[f"{algo}/{step}/{name}"] = p.detach().numpy().copy()
                out[f"{algo}/{step}/{name}@exp_avg"] = st["exp_avg"].numpy().copy()
                out[f"{algo}/{step}/{name}@exp_avg_sq"] = st["exp_avg_sq"].numpy().copy()
            print(algo, step, {k: float(v) for k, v in vals.items()})
    np.savez_compressed(U.GOLDEN, **out)
    print("wrote", U.GOLDEN, os.path.getsize(U.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
