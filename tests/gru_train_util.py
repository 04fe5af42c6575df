"""Cases, inputs and the tests' own restatements of the reference's GRULayer (algorithms/utils/gru.py) for the training GRU
(aircombat-selfplay_amd/gru_train.py), shared by tests/golden/make_gru_train_golden.py and the tests.

Every input comes from policy_util.hashed (an exact integer hash), so tests/golden/gru_train.npz holds only the reference's outputs
and gradients. They are stored as float32, plus one float64 projection per array (``<key>@p``: the dot product with a hashed vector)
that the float64 restatement is held to at 1e-12. The weight gradients are stored on DW_ROWS only (48 of the 384 gate rows, every
gate represented), which keeps the file small."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from policy_util import hashed

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gru_train.npz")
H = 128
# name -> (N chunks, T steps, mask pattern)
CASES = {
    "mix": (21, 8, "mix"),          # N not a multiple of the 16-row tile; zeros at t = 0, mid-chunk, and one step with every mask 0
    "long": (3, 60, "ones"),        # T = 60 with no zero at all
    "single": (1, 60, "sparse"),    # N = 1, T = 60, a few episode ends
    "t1": (7, 1, "sparse"),         # the T = 1 branch (x.size(0) == hxs.size(0))
}
KEYS = ("out", "h_T", "dx", "dhxs", "dW_ih", "dW_hh", "db_ih", "db_hh")
DW_ROWS = np.arange(0, 3 * H, 8) + np.arange(48) % 8


def masks(name):
    N, T, kind = CASES[name]
    if kind == "ones":
        return np.ones((T * N, 1), np.float32)
    u = hashed(7000 + len(name), T * N).reshape(T, N)
    m = (u > (-0.5 if kind == "mix" else -0.85)).astype(np.float32)
    if kind == "mix":
        m[0, ::3] = 0.0      # some rows start a new episode at t = 0
        m[0, 1::3] = 1.0
        m[4, :] = 0.0        # every row's episode ended at step 4
        m[5, :] = 1.0
    return m.reshape(T * N, 1)


def inputs(name):
    """float32 numpy inputs of a case: weights in state_dict layout, x [T*N, 128], hxs [N, 1, 128], masks [T*N, 1], and the upstream
    gradients g_out [T*N, 128] (of the layer's output, after the LayerNorm) and g_h [N, 1, 128] (of h_T)."""
    N, T, _ = CASES[name]
    k = 100 * (list(CASES).index(name) + 1)
    b = np.float32(1.0 / np.sqrt(H))
    return {"weight_ih_l0": (hashed(k + 1, 3 * H * H) * b).reshape(3 * H, H), "weight_hh_l0": (hashed(k + 2, 3 * H * H) * b).reshape(3 * H, H),
            "bias_ih_l0": hashed(k + 3, 3 * H) * b, "bias_hh_l0": hashed(k + 4, 3 * H) * b,
            "x": hashed(k + 5, T * N * H).reshape(T * N, H) * np.float32(2.0), "hxs": hashed(k + 6, N * H).reshape(N, 1, H),
            "masks": masks(name), "g_out": hashed(k + 7, T * N * H).reshape(T * N, H), "g_h": hashed(k + 8, N * H).reshape(N, 1, H)}


def projector(key, n):
    return hashed(9000 + KEYS.index(key), n).astype(np.float64)


def project(key, a):
    a = np.asarray(a, np.float64).ravel()
    return float(a @ projector(key, a.size))


def stored(key, a):
    """What the fixture keeps of result ``key``: the weight gradients on DW_ROWS, everything else whole."""
    a = np.asarray(a)
    return a[DW_ROWS] if key in ("dW_ih", "dW_hh") else a


def step_layer(p, x, hxs, masks, N, T):
    """The layer as a per-step loop in torch (any dtype, autograd): h_in = h * m_t at every step, torch's gate formula, then
    LayerNorm(128) with unit scale and zero shift. Returns (out [T*N, 128], h_T [N, 1, 128])."""
    h = hxs.reshape(N, H)
    xs, ms = x.reshape(T, N, H), masks.reshape(T, N, 1)
    ys = []
    for t in range(T):
        h = h * ms[t]
        gi = xs[t] @ p["weight_ih_l0"].T + p["bias_ih_l0"]
        gh = h @ p["weight_hh_l0"].T + p["bias_hh_l0"]
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        ys.append(h)
    y = torch.cat(ys)
    return F.layer_norm(y, (H,), eps=1e-5), h.reshape(N, 1, H)


def segment_layer(gru, norm, x, hxs, masks):
    """The reference's algorithm, restated: T = 1 when x and hxs have as many rows; otherwise the steps where any row's mask is 0 are
    found on the host (``nonzero().cpu()``, a synchronisation) and nn.GRU runs once per run of steps between them."""
    N = hxs.size(0)
    if x.size(0) == N:
        y, h = gru(x.unsqueeze(0), (hxs * masks.reshape(N, 1, 1)).transpose(0, 1).contiguous())
        return norm(y.squeeze(0)), h.transpose(0, 1)
    T = x.size(0) // N
    xs, ms = x.view(T, N, x.size(1)), masks.view(T, N)
    cuts = ((ms[1:] == 0.0).any(dim=-1).nonzero().squeeze(-1).cpu() + 1).tolist()
    cuts = [0] + cuts + [T]
    h = hxs.transpose(0, 1)
    outs = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        y, h = gru(xs[a:b], (h * ms[a].view(1, -1, 1)).contiguous())
        outs.append(y)
    return norm(torch.cat(outs).view(T * N, -1)), h.transpose(0, 1)


def run_with_grads(layer_fn, params, x, hxs, masks, g_out, g_h):
    """Forward + backward of loss = <out, g_out> + <h_T, g_h>; returns the KEYS as float64 numpy arrays. ``params`` are the four GRU
    tensors (leaf, requires_grad) as a dict in state_dict naming; x and hxs require grad."""
    out, h_T = layer_fn(x, hxs, masks)
    ((out * g_out).sum() + (h_T.reshape(g_h.shape) * g_h).sum()).backward()
    np64 = lambda t: t.detach().double().cpu().numpy()
    return {"out": np64(out), "h_T": np64(h_T).reshape(-1, H), "dx": np64(x.grad), "dhxs": np64(hxs.grad).reshape(-1, H),
            "dW_ih": np64(params["weight_ih_l0"].grad), "dW_hh": np64(params["weight_hh_l0"].grad),
            "db_ih": np64(params["bias_ih_l0"].grad), "db_hh": np64(params["bias_hh_l0"].grad)}


def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}
