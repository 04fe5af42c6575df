"""The PPO / MAPPO update's recurrent layer on the device ("The training GRU").

``DeviceGRULayer`` is a drop-in for the reference's ``GRULayer`` (algorithms/utils/gru.py) with the same children (``gru``, ``norm``)
and so the same state_dict keys. Its recurrence runs as two HIP kernels (csrc/gru_train.hpp), one launch per direction whatever T and
the mask pattern are, ordered on torch's current stream: no ``nonzero().cpu()``, no per-segment ``nn.GRU`` calls, no host
synchronisation. The dense products around it (``x W_ihᵀ``, ``dx``, ``dW_ih``, ``dW_hh``, the bias sums) and the LayerNorm stay torch.

``use_device_gru(policy)`` swaps every GRULayer-shaped child of a policy for a ``DeviceGRULayer`` reusing the same ``gru`` and ``norm``
submodules, so Parameter objects, optimiser state and checkpoints are unchanged.

``products`` (everywhere it appears) is how the two recurrence kernels multiply by ``W_hh``: ``"fp32"``, the default, on the fp32
matrix instruction; ``"bf16x3"`` with every value as three bf16 pieces and six piece products on the bf16 matrix instruction
(csrc/gru_train_split.hpp), as exact as fp32 to the tests' bound and shorter per step. Nothing else depends on it.
"""
import torch
import torch.nn as nn

from .policy import UnsupportedPolicy
from .train_common import PRODUCTS, Launch, products_code, swap_children   # noqa: F401  (PRODUCTS, products_code: also this module's names)

HID = 128
SAVED = 4 * HID   # floats per (step, row) the forward keeps for the backward: r, z, n, W_hn h + b_hn


class DeviceGRUFunction(torch.autograd.Function):
    """(x [T*N, 128], hxs [N, 128], masks [T*N], W_ih, W_hh, b_ih, b_hh) -> (y [T*N, 128] before the LayerNorm, h_T [N, 128]).

    Each step starts from ``h_{t-1} * m_t``. ``dhxs`` is computed only when ``hxs`` requires grad; nothing is saved when no input
    requires grad or grad mode is off (``apply`` is called through ``gru_seq``, which decides that: inside ``forward`` grad mode is
    always off and ``needs_input_grad`` ignores it)."""

    @staticmethod
    def forward(ctx, x, hxs, masks, w_ih, w_hh, b_ih, b_hh, save, products=0):
        N = hxs.shape[0]
        T = x.shape[0] // N
        x, hxs, masks, w_hh, b_hh = x.contiguous(), hxs.contiguous(), masks.contiguous(), w_hh.contiguous(), b_hh.contiguous()
        gi = torch.addmm(b_ih, x, w_ih.t())
        run = Launch(x)
        y, h_T = run.empty(T * N, HID), run.empty(N, HID)
        saved = run.empty(T * N, SAVED) if save else None
        run("ac_gru_seq_forward_p", N, T, gi, hxs, masks, w_hh, b_hh, y, h_T, saved, products)
        if save:
            ctx.save_for_backward(x, hxs, masks, w_ih, w_hh, y, saved)
            ctx.shape = (N, T)
            ctx.products = products
        ctx.set_materialize_grads(False)
        return y, h_T

    @staticmethod
    def backward(ctx, dy, dh_T):
        x, hxs, masks, w_ih, w_hh, y, saved = ctx.saved_tensors
        N, T = ctx.shape
        need = ctx.needs_input_grad
        run = Launch(x)
        dgi, dgh = run.empty(T * N, 3 * HID), run.empty(T * N, 3 * HID)
        dhxs = run.empty(N, HID) if need[1] else None
        dy = None if dy is None else dy.contiguous()
        dh_T = None if dh_T is None else dh_T.contiguous()
        run("ac_gru_seq_backward_p", N, T, dy, dh_T, saved, y, hxs, masks, w_hh, dgi, dgh, dhxs, ctx.products)
        dx = dgi @ w_ih if need[0] else None
        # the weight gradients as one batched GEMM over the steps (K = N each) and a sum over T: a single GEMM with K = T * N
        # accumulates in fp32 along the whole minibatch (measured 6.1e-6 relative against float64 at N = 4096, T = 60, torch's
        # per-segment path 3.6e-7); per step it is as accurate as torch's
        dw_ih = torch.bmm(dgi.view(T, N, 3 * HID).transpose(1, 2), x.view(T, N, HID)).sum(0) if need[3] else None
        dw_hh = None
        if need[4]:
            # h_in of every step, rebuilt from the outputs (not stored twice): [hxs, y_0 .. y_{T-2}] * m
            h_in = torch.cat([hxs.unsqueeze(0), y.view(T, N, HID)[:-1]]) * masks.view(T, N, 1)
            dw_hh = torch.bmm(dgh.view(T, N, 3 * HID).transpose(1, 2), h_in).sum(0)
        db_ih = dgi.sum(0) if need[5] else None
        db_hh = dgh.sum(0) if need[6] else None
        return (dx, dhxs, None, dw_ih, dw_hh, db_ih, db_hh, None, None)[:len(need)]


def gru_seq(x, hxs, masks, w_ih, w_hh, b_ih, b_hh, products="fp32"):
    """DeviceGRUFunction with its ``save`` decided here: grad mode on and some input requiring grad."""
    code = products_code(products)
    save = torch.is_grad_enabled() and any(t.requires_grad for t in (x, hxs, w_ih, w_hh, b_ih, b_hh))
    return DeviceGRUFunction.apply(x, hxs, masks, w_ih, w_hh, b_ih, b_hh, save, code)


def check_gru(gru, where="gru", device=True):
    """UnsupportedPolicy unless ``gru`` is what the kernels run: nn.GRU 128 -> 128, one layer, with bias, not batch-first, not
    bidirectional, float32 and, with ``device``, on a CUDA device."""
    if not isinstance(gru, nn.GRU):
        raise UnsupportedPolicy(f"{where}: not an nn.GRU ({type(gru).__name__})")
    bad = []
    if gru.input_size != HID or gru.hidden_size != HID:
        bad.append(f"sizes {gru.input_size} -> {gru.hidden_size} (only {HID} -> {HID})")
    if gru.num_layers != 1:
        bad.append(f"{gru.num_layers} layers (only 1)")
    if not gru.bias:
        bad.append("no bias")
    if gru.batch_first:
        bad.append("batch_first")
    if gru.bidirectional:
        bad.append("bidirectional")
    if getattr(gru, "proj_size", 0):
        bad.append("proj_size")
    w = gru.weight_hh_l0
    if w.dtype != torch.float32:
        bad.append(f"dtype {w.dtype} (only float32)")
    if device and w.device.type != "cuda":
        bad.append(f"device {w.device} (only a CUDA device)")
    if bad:
        raise UnsupportedPolicy(f"{where}: " + ", ".join(bad))


class DeviceGRULayer(nn.Module):
    """GRULayer(input_size, hidden_size, num_layers) of the reference with the recurrence on the device: children ``gru`` (nn.GRU) and
    ``norm`` (nn.LayerNorm), forward(x, hxs, masks) -> (norm(y), h_T [N, 1, 128]). ``x.size(0) == hxs.size(0)`` means T = 1, as there.
    Given ``gru`` / ``norm``, those modules are used as they are (use_device_gru). ``products`` ("fp32" or "bf16x3", kept as
    ``layer.products``) selects the recurrence kernels' product."""

    def __init__(self, input_size=HID, hidden_size=HID, num_layers=1, gru=None, norm=None, products="fp32"):
        super().__init__()
        products_code(products)
        self.products = products
        self._hidden_size = hidden_size
        self._num_layers = num_layers
        self.gru = gru if gru is not None else nn.GRU(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers)
        self.norm = norm if norm is not None else nn.LayerNorm(hidden_size)

    def forward(self, x, hxs, masks):
        g = self.gru
        check_gru(g, type(self).__name__ + ".gru")
        N = hxs.size(0)
        T = 1 if x.size(0) == N else x.size(0) // N
        if T * N != x.size(0):
            raise ValueError(f"x has {x.size(0)} rows, not a multiple of hxs' {N}")
        y, h_T = gru_seq(x, hxs.reshape(N, HID), masks.reshape(T * N).to(torch.float32), g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0,
                         g.bias_hh_l0, self.products)
        return self.norm(y), h_T.view(N, 1, HID)

    @property
    def output_size(self):
        return self._hidden_size


def check_one_layer(layer, where):
    if getattr(layer, "_num_layers", 1) != 1:
        raise UnsupportedPolicy(f"{where}: {layer._num_layers} layers (only 1)")


def same_children(cls, layer, products="fp32"):
    """``cls`` (DeviceGRULayer or a subclass) holding the very ``gru`` and ``norm`` of ``layer``."""
    return cls(layer.gru.input_size, layer.gru.hidden_size, layer.gru.num_layers, gru=layer.gru, norm=layer.norm, products=products)


def _gru_layer_shaped(m):
    return not isinstance(m, DeviceGRULayer) and isinstance(getattr(m, "gru", None), nn.GRU) and isinstance(getattr(m, "norm", None), nn.LayerNorm)


def use_device_gru(module, products="fp32"):
    """Swap every GRULayer-shaped child (a module with an nn.GRU ``gru`` and an nn.LayerNorm ``norm``) of ``module`` for a
    DeviceGRULayer holding the same two submodules. ``module`` is an nn.Module (``policy.actor``, ``policy.critic``) or an object with
    ``actor`` / ``critic`` modules (the reference's PPO and MAPPO ``PPOPolicy``). Every layer is checked before any is swapped; an
    unsupported one raises UnsupportedPolicy naming it. Every new layer gets ``products``; one that is neither "fp32" nor "bf16x3" is a
    ValueError before anything is looked at. Returns the number of layers swapped."""
    products_code(products)

    def check(child, where):
        check_gru(child.gru, where + ".gru")
        check_one_layer(child, where)
    return swap_children(module, _gru_layer_shaped, check, lambda child: same_children(DeviceGRULayer, child, products), "a GRULayer")
