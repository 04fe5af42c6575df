"""The split-bf16 form of the training MLP blocks (csrc/mlp_train_split.hpp, products="bf16x3"), emulated on the CPU with
gru_split_util.split_product, and what the new tests share.

The three products of a block: z = x Wᵀ (K zero-padded to whole k-steps of 32, which adds exact zeros), dx = dz W (K = 128 units) and
dW = dzᵀ x, whose sum runs over the rows: a workgroup keeps one fp32 accumulator per result over the 32-row tiles it walks, one k-step
per tile, and the shares of the workgroups are added in fp32 afterwards. At the sizes of mlp_train_util.CASES every workgroup walks one
tile, so the emulation forms dW per tile and adds the tiles in fp32. Everything that is not a product (bias, ReLU, LayerNorm and its
backward, db, dgamma, dbeta) is torch fp32. The emulation has the kernels' terms, pieces and number of fp32 roundings per accumulator
(the kernel's dx spreads its terms over three accumulators, one per order, which the single one here does not flatter); it is not
bit-exact to the device (gru_split_util)."""
import numpy as np
import torch
import torch.nn.functional as F

import mlp_train_util as U
from gru_split_util import SIX, THREE, bound, rel, split_product  # noqa: F401  (shared with the tests)

H = U.H
PRODUCTS = ("fp32", "bf16x3")
PRODUCT_CODES = {"fp32": 0, "bf16x3": 1}
KP_ALL = 32 | 64 | 128 | 256


def split_kp(K):
    """The padded K of the split form: a k-step is 32."""
    return 32 if K <= 32 else 64 if K <= 64 else 128 if K <= 128 else 256


def _pad_k(a):
    return np.ascontiguousarray(np.pad(a, ((0, 0), (0, (-a.shape[1]) % 32))))


class SplitLinear(torch.autograd.Function):
    """x [n, K] @ w [128, K]ᵀ with the three products of the block in the split form (``terms``), fp32 in and out."""

    @staticmethod
    def forward(ctx, x, w, terms):
        ctx.save_for_backward(x, w)
        ctx.terms = terms
        return torch.from_numpy(split_product(_pad_k(x.detach().numpy()), _pad_k(w.detach().numpy()), terms))

    @staticmethod
    def backward(ctx, dz):
        x, w = (t.detach().numpy() for t in ctx.saved_tensors)
        dz = np.ascontiguousarray(dz.numpy())
        dx = split_product(dz, np.ascontiguousarray(w.T), ctx.terms)     # the sum runs over the 128 units: 4 k-steps
        pad = (-x.shape[0]) % 32
        dzp, xp = np.pad(dz, ((0, pad), (0, 0))), np.pad(x, ((0, pad), (0, 0)))
        dw = np.zeros(w.shape, np.float32)
        for r in range(0, xp.shape[0], 32):   # one tile = one k-step = one workgroup's share here; the shares are added in fp32
            dw = dw + split_product(np.ascontiguousarray(dzp[r:r + 32].T), np.ascontiguousarray(xp[r:r + 32].T), ctx.terms)
        return torch.from_numpy(dx), torch.from_numpy(dw), None


def _tensors(name, dtype):
    inp = U.inputs(name)
    p = {k: torch.tensor(inp[k], dtype=dtype, requires_grad=True) for k in U.PNAMES}
    x = torch.tensor(inp["x"], dtype=dtype, requires_grad=U.CASES[name][2])
    return p, x, torch.tensor(inp["g_out"], dtype=dtype)


def _layer_fn(p, product, zs):
    def block(x, lin, ln):
        z = product(x, p[lin + ".weight"]) + p[lin + ".bias"]
        zs.append(z.detach().double().numpy())
        return F.layer_norm(torch.relu(z), (H,), p[ln + ".weight"], p[ln + ".bias"], U.EPS)
    def fn(x):
        y0 = block(x, "fc.0", "fc.2")
        return y0, block(y0, "fc.3", "fc.5")
    return fn


_runs = {}


def emulated(name, form):
    """(results as mlp_train_util.run_with_grads gives them, [z of block 0, z of block 1] as float64 numpy) of a case in ``form``:
    "f64" (everything float64: the reference), "fp32" (torch fp32), "six" or "three" (the split products). Computed once."""
    if (name, form) not in _runs:
        p, x, g_out = _tensors(name, torch.float64 if form == "f64" else torch.float32)
        if form in ("f64", "fp32"):
            product = lambda a, w: a @ w.T
        else:
            terms = SIX if form == "six" else THREE
            product = lambda a, w: SplitLinear.apply(a, w, terms)
        zs = []
        _runs[(name, form)] = (U.run_with_grads(_layer_fn(p, product, zs), p, x, g_out), zs)
    return _runs[(name, form)]


def edge_inputs(M, K, seed=0):
    """A two-block layer K -> 128 -> 128 at any size, float32 numpy in mlp_train_util.inputs' naming: x standard normal, W ~ N(0, 1/K),
    b ~ 0.1 N, gamma and beta away from 1 and 0."""
    rng = np.random.default_rng(1000 * K + M + seed)
    rn = lambda *s: rng.standard_normal(s).astype(np.float32)
    return {"fc.0.weight": rn(H, K) / np.float32(np.sqrt(K)), "fc.0.bias": np.float32(0.1) * rn(H), "fc.2.weight": 1 + np.float32(0.3) * rn(H),
            "fc.2.bias": np.float32(0.3) * rn(H), "fc.3.weight": rn(H, H) / np.float32(np.sqrt(H)), "fc.3.bias": np.float32(0.1) * rn(H),
            "fc.5.weight": 1 + np.float32(0.3) * rn(H), "fc.5.bias": np.float32(0.3) * rn(H), "x": rn(M, K), "g_out": rn(M, H)}
