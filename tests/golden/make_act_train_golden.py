"""Generate tests/golden/act_train.npz from the REFERENCE's own ACTLayer (algorithms/utils/act.py; runs only where the reference tree
exists, named by AC_REFERENCE_ROOT).

For every case of tests/act_train_util.CASES an ``ACTLayer(space, 128, "", 1, 0.01)`` (no act MLP) runs in float64 on the CPU with the
case's hashed parameters: ``evaluate_actions``, then backward of <action_log_probs, g1> + <dist_entropy, g2>. Stored per case
(``<case>/<key>``): action_log_probs, dist_entropy and the gradients of x and of every head that takes part, as float32, each with its
float64 projection ``<case>/<key>@p``. The inputs are not stored: the tests regenerate them. Only data is stored; no reference source
text. act.py imports gymnasium, which is stubbed with classes that carry what ACTLayer reads of a space (nvec, shape, n, indexing).
Before anything is written every case is also run in float32 and both runs are checked to be finite, and the munition heads that the
reference leaves out are checked to have got no gradient.

    AC_REFERENCE_ROOT=<reference checkout> python tests/golden/make_act_train_golden.py
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
import act_train_util as U  # noqa: E402

if "gymnasium" not in sys.modules:
    g, sp = types.ModuleType("gymnasium"), types.ModuleType("gymnasium.spaces")
    for n in ("Box", "Discrete", "MultiDiscrete", "MultiBinary", "Dict", "Space"):
        setattr(sp, n, type(n, (), {}))
    sp.Tuple = type("Tuple", (tuple,), {})
    g.spaces, g.Space = sp, sp.Space
    sys.modules.update({"gymnasium": g, "gymnasium.spaces": sp})
import gymnasium  # noqa: E402
from algorithms.utils.act import ACTLayer  # noqa: E402


def space(nvec, ns):
    S = gymnasium.spaces

    def multi(v):
        m = S.MultiDiscrete()
        m.nvec, m.shape = np.array(v), (len(v),)
        return m
    if ns == 0:
        return multi(nvec)
    second = S.Discrete()
    second.n = 2
    return S.Tuple((multi(nvec), second if ns == 1 else multi([2] * 4)))


def run(name, dtype):
    M, nvec, ns, _ = U.CASES[name]
    inp = U.inputs(name)
    layer = ACTLayer(space(nvec, ns), U.H, "", 1, 0.01).to(dtype)
    assert list(layer.state_dict()) == U.pnames(name), list(layer.state_dict())
    layer.load_state_dict({k: torch.from_numpy(inp[k]).to(dtype) for k in U.pnames(name)})
    x = torch.tensor(inp["x"], dtype=dtype, requires_grad=True)
    res, unused = U.run_with_grads(layer.evaluate_actions, dict(layer.named_parameters()), x, inp, name)
    assert unused == [i for i in range(U.n_heads(name)) if i not in U.used_heads(name)], (name, unused)
    assert all(np.isfinite(v).all() for v in res.values()), (name, dtype)
    return res


def main():
    out = {}
    for name in U.CASES:
        run(name, torch.float32)          # finite in float32 too (the sharp case above all)
        res = run(name, torch.float64)
        for k in U.keys(name):
            out[f"{name}/{k}"] = res[k].astype(np.float32)
            out[f"{name}/{k}@p"] = np.float64(U.project(k, res[k]))
    np.savez(U.GOLDEN, **out)
    print(U.GOLDEN, os.path.getsize(U.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
