"""The PPO / MAPPO update's whole recurrent layer on the device ("The whole GRU layer").

``DeviceFusedGRULayer`` is ``DeviceGRULayer`` (gru_train.py) with nothing left to torch: the input product ``x W_ihᵀ + b_ih``, the
recurrence, the LayerNorm and, backward, the LayerNorm's gradients, ``dx``, ``dW_ih``, ``dW_hh`` and the bias sums are HIP kernels
(csrc/gru_layer_train.hpp around the recurrence kernels of csrc/gru_train.hpp), queued by one C call per direction on torch's current
stream. It has the same children (``gru``, ``norm``), so the same Parameter objects and state_dict keys.

``use_device_gru_layer(policy)`` swaps every GRULayer-shaped child of a policy, and every ``DeviceGRULayer`` that ``use_device_gru``
put there, for a ``DeviceFusedGRULayer`` holding the same two submodules. Nothing selects it unless the caller asks.

``products`` ("fp32", the default, or "bf16x3": gru_train.py) selects the product of the two recurrence kernels alone; the input product,
the LayerNorm and the weight and input gradients are the same kernels either way.

``dense_products`` ("fp32", the default, or "bf16x3"), independent of it, selects how the layer's three dense products are formed:
``gi = x W_ihᵀ``, ``dx = dgi W_ih`` and the weight gradients ``dW_ih``, ``dW_hh``. "bf16x3" takes them with every value as three bf16
pieces and six piece products on the bf16 matrix instruction (csrc/gru_layer_train_split.hpp), within the tests' bound of fp32;
``W_ih`` stays the caller's fp32 tensor, split at every call, and the bias gradients stay fp32 sums.
"""
import torch

from . import gru_train
from .gru_train import HID, SAVED, DeviceGRULayer
from .policy import UnsupportedPolicy
from .train_common import Launch, layernorm_faults, products_code, swap_children


class DeviceGRULayerFunction(torch.autograd.Function):
    """(x [T*N, 128], hxs [N, 128], masks [T*N], W_ih, W_hh, b_ih, b_hh, gamma, beta, eps, save) -> (out [T*N, 128] after the
    LayerNorm, h_T [N, 128]).

    Each step starts from ``h_{t-1} * m_t``. With ``save`` the forward keeps the recurrence's outputs and gates and each row's mean
    and 1/std; ``apply`` is called through ``gru_layer``, which decides that (inside ``forward`` grad mode is always off and
    ``needs_input_grad`` ignores it). The backward computes ``dx`` and ``dhxs`` only when asked, and returns a parameter's gradient
    only where ``needs_input_grad`` asks."""

    @staticmethod
    def forward(ctx, x, hxs, masks, w_ih, w_hh, b_ih, b_hh, gamma, beta, eps, save, products=0, dense_products=0):
        N = hxs.shape[0]
        T = x.shape[0] // N
        x, hxs, masks, w_ih, w_hh, b_ih, b_hh, gamma, beta = (t.contiguous() for t in (x, hxs, masks, w_ih, w_hh, b_ih, b_hh, gamma, beta))
        run = Launch(x)
        # the gate pre-activations live in a torch tensor: torch's allocator orders its reuse on this stream
        ws = run.empty(T * N * 3 * HID)
        out, h_T, y = run.empty(T * N, HID), run.empty(N, HID), run.empty(T * N, HID)
        saved, stats = (run.empty(T * N, SAVED), run.empty(T * N, 2)) if save else (None, None)
        run("ac_gru_layer_forward_pd", N, T, x, hxs, masks, w_ih, w_hh, b_ih, b_hh, gamma, beta, eps, ws, out, h_T, y, saved, stats, products,
            dense_products)
        if save:
            ctx.save_for_backward(x, hxs, masks, w_ih, w_hh, gamma, y, saved, stats)
            ctx.shape = (N, T)
            ctx.products, ctx.dense_products = products, dense_products   # the backward uses what the forward ran with
        ctx.set_materialize_grads(False)
        return out, h_T

    @staticmethod
    def backward(ctx, g_out, g_h):
        x, hxs, masks, w_ih, w_hh, gamma, y, saved, stats = ctx.saved_tensors
        N, T = ctx.shape
        need = ctx.needs_input_grad
        run = Launch(x)
        new = run.empty
        ws = run.workspace("ac_gru_layer_workspace_floats", N, T)
        dx = new(T * N, HID) if need[0] else None
        dhxs = new(N, HID) if need[1] else None
        dw_ih, dw_hh, db_ih, db_hh, dgamma, dbeta = new(3 * HID, HID), new(3 * HID, HID), new(3 * HID), new(3 * HID), new(HID), new(HID)
        g_out = None if g_out is None else g_out.contiguous()
        g_h = None if g_h is None else g_h.contiguous()
        run("ac_gru_layer_backward_pd", N, T, g_out, g_h, x, hxs, masks, w_ih, w_hh, gamma, y, saved, stats, ws, dx, dhxs, dw_ih, dw_hh, db_ih,
            db_hh, dgamma, dbeta, ctx.products, ctx.dense_products)
        grads = (dx, dhxs, None, dw_ih, dw_hh, db_ih, db_hh, dgamma, dbeta, None, None, None, None)
        return tuple(g if n else None for g, n in zip(grads, need))


def dense_products_code(dense_products):
    """train_common.products_code for the argument ``dense_products``."""
    return products_code(dense_products, "dense_products")


def gru_layer(x, hxs, masks, w_ih, w_hh, b_ih, b_hh, gamma, beta, eps=1e-5, products="fp32", dense_products="fp32"):
    """The whole layer as a function: DeviceGRULayerFunction with its ``save`` decided here (grad mode on and some input requiring
    grad). x [T*N, 128], hxs [N, 128], masks [T*N], float32 on one CUDA device -> (out [T*N, 128], h_T [N, 128]). ``products`` selects
    the recurrence kernels' product, ``dense_products`` that of gi, dx and the weight gradients."""
    code, dense = products_code(products), dense_products_code(dense_products)
    for name, t in (("x", x), ("hxs", hxs), ("masks", masks)):   # no torch op inside would notice: the kernels read float32 as given
        if t.dtype != torch.float32 or t.device != w_ih.device:
            raise UnsupportedPolicy(f"gru_layer: {name} is {t.dtype} on {t.device} (only float32 on {w_ih.device})")
    if x.dim() != 2 or x.shape[1] != HID or tuple(hxs.shape[1:]) != (HID,) or hxs.shape[0] < 1 or x.shape[0] % hxs.shape[0] or masks.numel() != x.shape[0]:
        raise ValueError(f"gru_layer: x {tuple(x.shape)}, hxs {tuple(hxs.shape)}, masks {tuple(masks.shape)} are not [T*N, {HID}], [N, {HID}], [T*N]")
    save = torch.is_grad_enabled() and any(t.requires_grad for t in (x, hxs, w_ih, w_hh, b_ih, b_hh, gamma, beta))
    return DeviceGRULayerFunction.apply(x, hxs, masks, w_ih, w_hh, b_ih, b_hh, gamma, beta, float(eps), save, code, dense)


def check_layer(gru, norm, where="rnn", device=True):
    """UnsupportedPolicy unless (gru, norm) is what the kernels run: whatever check_gru accepts, then nn.LayerNorm((128,)) with affine
    parameters, float32 and, with ``device``, on a CUDA device."""
    said = []   # everything wrong with the layer in one message: the GRU's part as check_gru words it, then the LayerNorm's
    try:
        if device:   # the call as it was before ``device`` existed: callers and tests that stand in for check_gru take two arguments
            gru_train.check_gru(gru, where + ".gru")
        else:
            gru_train.check_gru(gru, where + ".gru", device=False)
    except UnsupportedPolicy as exc:
        said.append(str(exc))
    bad = layernorm_faults(norm, device)
    if bad:
        said.append(f"{where}.norm: " + ", ".join(bad))
    if said:
        raise UnsupportedPolicy("; ".join(said))


class DeviceFusedGRULayer(DeviceGRULayer):
    """DeviceGRULayer with the whole layer on the device: the same children ``gru`` and ``norm``, the same forward(x, hxs, masks) ->
    (out, h_T [N, 1, 128]) and the same T = 1 rule when ``x.size(0) == hxs.size(0)``, as one autograd function with no torch op
    inside. ``dense_products`` ("fp32" or "bf16x3", kept as ``layer.dense_products``) selects the product of gi, dx and the weight
    gradients, as ``products`` selects the recurrence kernels'."""

    def __init__(self, *args, dense_products="fp32", **kw):
        dense_products_code(dense_products)
        super().__init__(*args, **kw)
        self.dense_products = dense_products

    def forward(self, x, hxs, masks):
        g, ln = self.gru, self.norm
        check_layer(g, ln, type(self).__name__)
        N = hxs.size(0)
        T = 1 if x.size(0) == N else x.size(0) // N
        if T * N != x.size(0):
            raise ValueError(f"x has {x.size(0)} rows, not a multiple of hxs' {N}")
        out, h_T = gru_layer(x, hxs.reshape(N, HID), masks.reshape(T * N).to(torch.float32), g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0,
                             g.bias_hh_l0, ln.weight, ln.bias, ln.eps, self.products, self.dense_products)
        return out, h_T.view(N, 1, HID)


def _swappable(m):
    if isinstance(m, DeviceFusedGRULayer):
        return False
    return isinstance(m, DeviceGRULayer) or gru_train._gru_layer_shaped(m)


def use_device_gru_layer(module, products=None, dense_products=None):
    """Swap every GRULayer-shaped child of ``module`` (a module with an nn.GRU ``gru`` and an nn.LayerNorm ``norm``), and every
    DeviceGRULayer that use_device_gru put there, for a DeviceFusedGRULayer holding the same two submodules. ``module`` is an nn.Module
    (``policy.actor``, ``policy.critic``) or an object with ``actor`` / ``critic`` modules. Every layer is checked before any is
    swapped; an unsupported one raises UnsupportedPolicy naming it. ``products`` is "fp32" (what None means for a layer that was not a
    DeviceGRULayer) or "bf16x3"; a DeviceGRULayer keeps its own unless one is given here. Anything else is a ValueError before a module
    is touched. ``dense_products`` likewise: None keeps a DeviceFusedGRULayer's own (one that is handed in as the module's child stays as
    it is: only other layers are swapped) and means "fp32" for anything else. Returns the number of layers swapped."""
    if products is not None:
        products_code(products)
    if dense_products is not None:
        dense_products_code(dense_products)

    def check(child, where):
        check_layer(child.gru, child.norm, where)
        gru_train.check_one_layer(child, where)

    def build(child):
        own = products if products is not None else getattr(child, "products", "fp32") if isinstance(child, DeviceGRULayer) else "fp32"
        dense = dense_products if dense_products is not None else getattr(child, "dense_products", "fp32")
        return gru_train.same_children(lambda *a, **kw: DeviceFusedGRULayer(*a, dense_products=dense, **kw), child, own)
    return swap_children(module, _swappable, check, build, "a GRULayer")
