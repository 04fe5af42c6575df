"""Generate tests/golden/mlp_train.npz from the REFERENCE's own MLPLayer (algorithms/utils/mlp.py; runs only where the reference tree
exists, named by AC_REFERENCE_ROOT).

For every case of tests/mlp_train_util.CASES an ``MLPLayer(K, "128 128", 1)`` runs in float64 on the CPU with the case's hashed
parameters: forward, then backward of <out, g_out> with the hashed upstream gradient. Stored per case (``<case>/<key>``): both blocks'
outputs and the gradients of each block's input, W, b, gamma and beta as float32 (on the rows mlp_train_util.stored keeps), each with
its float64 projection ``<case>/<key>@p``. The inputs are not stored: the tests regenerate them. Only data is stored; no reference
source text. mlp.py imports the observation flattener and with it gymnasium, which is stubbed: the layer itself never touches it.

    AC_REFERENCE_ROOT=<reference checkout> python tests/golden/make_mlp_train_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ["AC_REFERENCE_ROOT"]
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)
import mlp_train_util as U  # noqa: E402

if "gymnasium" not in sys.modules:
    g, sp = types.ModuleType("gymnasium"), types.ModuleType("gymnasium.spaces")
    for n in ("Box", "Discrete", "MultiDiscrete", "MultiBinary", "Tuple", "Dict", "Space"):
        setattr(sp, n, type(n, (), {}))
    g.spaces, g.Space = sp, sp.Space
    sys.modules.update({"gymnasium": g, "gymnasium.spaces": sp})
from algorithms.utils.mlp import MLPLayer  # noqa: E402


def main():
    out = {}
    for name, (M, K, x_grad) in U.CASES.items():
        inp = U.inputs(name)
        layer = MLPLayer(K, "128 128", 1).double()
        assert list(layer.state_dict()) == list(U.PNAMES)
        layer.load_state_dict({k: torch.from_numpy(inp[k].astype(np.float64)) for k in U.PNAMES})
        params = dict(layer.named_parameters())
        x = torch.tensor(inp["x"], dtype=torch.float64, requires_grad=x_grad)
        res = U.run_with_grads(U.module_layer_fn(layer), params, x, torch.tensor(inp["g_out"], dtype=torch.float64))
        for k in U.keys(name):
            s = U.stored(k, res[k])
            out[f"{name}/{k}"] = s.astype(np.float32)
            out[f"{name}/{k}@p"] = np.float64(U.project(k, s))
    np.savez(U.GOLDEN, **out)
    print(U.GOLDEN, os.path.getsize(U.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
