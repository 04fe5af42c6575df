"""Generate tests/golden/gru_train.npz from the REFERENCE's own GRULayer (algorithms/utils/gru.py; runs only where the reference tree
exists, named by AC_REFERENCE_ROOT).

For every case of tests/gru_train_util.CASES the layer runs in float64 on the CPU: forward, then backward of <out, g_out> + <h_T, g_h>
with the hashed upstream gradients. Stored per case (``<case>/<key>``): the layer's output (after its LayerNorm), h_T, and the gradients
of x, hxs, W_ih, W_hh, b_ih, b_hh as float32 (the weight gradients on gru_train_util.DW_ROWS), each with its float64 projection
``<case>/<key>@p``. The inputs are not stored: the tests regenerate them. Only data is stored; no reference source text.

    AC_REFERENCE_ROOT=<reference checkout> python tests/golden/make_gru_train_golden.py
"""
import os
import sys

import numpy as np
import torch

REF = os.environ["AC_REFERENCE_ROOT"]
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)
import gru_train_util as U  # noqa: E402
from algorithms.utils.gru import GRULayer  # noqa: E402


def main():
    out = {}
    for name in U.CASES:
        inp = U.inputs(name)
        layer = GRULayer(128, 128, 1).double()
        with torch.no_grad():
            for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
                getattr(layer.gru, k).copy_(torch.from_numpy(inp[k].astype(np.float64)))
        t = lambda k, g=False: torch.tensor(inp[k], dtype=torch.float64, requires_grad=g)
        params = {k: getattr(layer.gru, k) for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")}
        res = U.run_with_grads(layer, params, t("x", True), t("hxs", True), t("masks"), t("g_out"), t("g_h"))
        for k in U.KEYS:
            s = U.stored(k, res[k])
            out[f"{name}/{k}"] = s.astype(np.float32)
            out[f"{name}/{k}@p"] = np.float64(U.project(k, s))
    np.savez(U.GOLDEN, **out)
    print(U.GOLDEN, os.path.getsize(U.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
