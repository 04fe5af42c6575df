"""The split-bf16 form of the fused GRU layer's three dense products (csrc/gru_layer_train_split.hpp, dense_products="bf16x3"),
emulated on the CPU with gru_split_util.split_product, and what the new tests share.

The products: gi = x W_ihᵀ (K = 128), dx = dgi W_ih (K = 384) and dW_ih = dgiᵀ x, whose sum runs over the rows: one workgroup of
gru_dw_b3 keeps a single fp32 accumulator per result over its own share of the rows, a 32-row tile per k-step, so the emulation takes
a share (128 or 1920 rows, what a workgroup walks at 16 384 and 245 760 rows), zero-padded to whole tiles. The emulation has the
kernels' terms, pieces and number of fp32 roundings per accumulator (gru_dx_b3 spreads its terms over three accumulators, which the
single one here does not flatter); it is not bit-exact to the device (gru_split_util)."""
import numpy as np
import torch

from gru_split_util import SIX, THREE, bound, rel, split_product  # noqa: F401  (shared with the tests)

H, G = 128, 384
SEEDS = (0, 1, 2)
PRODUCT_ROWS = (33, 96)    # gi and dx
SHARE_ROWS = (128, 1920)   # dW: the rows one workgroup sums


def inputs(M, seed):
    """x standard normal, W_ih uniform in +-1/sqrt(128), dgi normal * 1e-2, float32."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, H)).astype(np.float32)
    w_ih = rng.uniform(-1.0, 1.0, (G, H)).astype(np.float32) / np.float32(np.sqrt(H))
    dgi = (rng.standard_normal((M, G)) * 1e-2).astype(np.float32)
    return x, w_ih, dgi


def operands(what, M, seed):
    """(a [n, K], w [m, K]) with the product a wᵀ, K the summed index."""
    x, w_ih, dgi = inputs(M, seed)
    if what == "gi":
        return x, w_ih
    if what == "dx":
        return dgi, np.ascontiguousarray(w_ih.T)
    pad = (-M) % 32   # dW: rows are the summed index, whole 32-row tiles
    return (np.ascontiguousarray(np.pad(dgi, ((0, pad), (0, 0))).T), np.ascontiguousarray(np.pad(x, ((0, pad), (0, 0))).T))


_errors = {}


def errors(what, M, seed):
    """rel against float64 of torch fp32, the six-term and the three-term product, computed once."""
    key = (what, M, seed)
    if key not in _errors:
        a, w = operands(what, M, seed)
        ref = a.astype(np.float64) @ w.astype(np.float64).T
        fp32 = (torch.from_numpy(a) @ torch.from_numpy(w).T).numpy()
        _errors[key] = {"fp32": rel(fp32, ref), "six": rel(split_product(a, w, SIX), ref), "three": rel(split_product(a, w, THREE), ref)}
    return _errors[key]
