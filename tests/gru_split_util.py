"""The split-bf16 product of the training GRU's recurrence kernels (csrc/gru_train_split.hpp, products="bf16x3"), emulated on the CPU,
and what the new tests share.

A value is split as the kernels split it: b0 = bf16(x), b1 = bf16(x - b0), b2 = bf16(x - b0 - b1), each rounded to nearest-even; the
subtractions are exact in fp32 and b0 + b1 + b2 = x. A product keeps the terms b_i(a) b_j(w) listed in ``SIX`` (i + j <= 2, smallest
first, the kernels' order) or, to show what the bound can tell apart, only the ``THREE`` largest. Per 32 k and term the exact piece
products are summed (in float64, which holds them exactly) and the sum is rounded into an fp32 accumulator: that is one matrix
instruction as far as it is documented. The order in which the matrix core adds the 32 products and the accumulator inside one
instruction is not known, so the emulation is not bit-exact to the device; it has the same terms, the same pieces and the same number
of fp32 roundings per accumulator."""
import numpy as np
import torch

import gru_train_util as GU

H = GU.H
FLOOR = 2.0 ** -20
SIX = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))
THREE = ((1, 0), (0, 1), (0, 0))


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def bound(e_ref):
    """The project's bound (tests/test_gpu_gru_train.py): four times torch fp32's own error, or 2^-20."""
    return max(4 * e_ref, FLOOR)


def bf16_round(x):
    """float32 -> the nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split3(x):
    x = np.asarray(x, np.float32)
    b0 = bf16_round(x)
    r1 = x - b0
    b1 = bf16_round(r1)
    b2 = bf16_round(r1 - b1)
    return b0, b1, b2


def split_product(a, w, terms=SIX):
    """a [n, K] @ w [m, K]ᵀ in fp32 with the split product: one fp32 accumulator per output, K in steps of 32, ``terms`` per step."""
    pa, pw = [p.astype(np.float64) for p in split3(a)], [p.astype(np.float64) for p in split3(w)]
    acc = np.zeros((a.shape[0], w.shape[0]), np.float32)
    for k in range(0, a.shape[1], 32):
        for i, j in terms:
            acc = (acc.astype(np.float64) + pa[i][:, k:k + 32] @ pw[j][:, k:k + 32].T).astype(np.float32)
    return acc


def recurrence(inp, N, T, product="f64"):
    """The recurrence as the kernels run it, without the LayerNorm: (y [T*N, 128], h_T [N, 128]) as float64 numpy. ``product`` is how
    h_in W_hhᵀ is formed: "f64" (everything in float64: the reference), "fp32" (torch's fp32 matmul; everything else fp32, as below),
    "six" or "three" (split_product; gates, biases and the input product in torch fp32)."""
    dt = torch.float64 if product == "f64" else torch.float32
    c = lambda k: torch.tensor(inp[k], dtype=dt)
    w_ih, w_hh, b_ih, b_hh = c("weight_ih_l0"), c("weight_hh_l0"), c("bias_ih_l0"), c("bias_hh_l0")
    xs, ms, h = c("x").reshape(T, N, H), c("masks").reshape(T, N, 1), c("hxs").reshape(N, H)
    ys = []
    for t in range(T):
        h = h * ms[t]
        gi = xs[t] @ w_ih.T + b_ih
        if product in ("f64", "fp32"):
            gh = h @ w_hh.T
        else:
            gh = torch.from_numpy(split_product(h.numpy(), w_hh.numpy(), SIX if product == "six" else THREE))
        gh = gh + b_hh
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        ys.append(h)
    return torch.cat(ys).double().numpy(), h.double().numpy()


def layer_norm64(y, eps=1e-5):
    y = np.asarray(y, np.float64)
    mu, var = y.mean(-1, keepdims=True), y.var(-1, keepdims=True)
    return (y - mu) / np.sqrt(var + eps)
