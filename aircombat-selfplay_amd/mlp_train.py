"""The PPO / MAPPO update's MLP layers on the device ("The training MLP blocks").

``DeviceMLPLayer`` is a drop-in for the reference's ``MLPLayer`` (algorithms/utils/mlp.py) with the same single child ``fc``
(``nn.Sequential`` of ``Linear, ReLU, LayerNorm`` triples) and so the same state_dict keys. Each triple runs as one fused HIP kernel
forward and one backward (csrc/mlp_train.hpp) on torch's current stream: ``y = LayerNorm(relu(x Wᵀ + b))`` without ``z`` or
``relu(z)`` ever reaching memory, and a backward that recomputes ``z`` and sums the parameter gradients in a fixed order.

``use_device_mlp(policy)`` swaps every MLPLayer-shaped module of a policy for a ``DeviceMLPLayer`` reusing the same ``fc``, so
Parameter objects, optimiser state and checkpoints are unchanged. It composes with ``use_device_gru`` in either order. The optional
``feature_norm``, the GRU layer's ``norm``, the heads, the loss and the optimiser stay torch.

``products="bf16x3"`` (``mlp_block``, ``DeviceMLPLayer``, ``use_device_mlp``) forms the blocks' three products from three bf16 pieces
per value on the bf16 matrix instruction (csrc/mlp_train_split.hpp); the default ``"fp32"`` runs the fp32 kernels as before.
"""
import torch
import torch.nn as nn

from .policy import UnsupportedPolicy
from .train_common import Launch, layernorm_faults, linear_faults, products_code, swap_children

HID = 128      # out-features of every block, the LayerNorm's width
K_MAX = 256    # in-features at most


class DeviceMLPBlockFunction(torch.autograd.Function):
    """(x [M, K], W [128, K], b, gamma, beta [128], eps, save[, products]) -> y [M, 128] = LayerNorm(relu(x Wᵀ + b)) * gamma + beta.

    With ``save`` the forward also keeps the rows' mean and 1/std (8 bytes per row) and the backward recomputes ``z`` from ``x``.
    ``dx`` is computed only when ``x`` requires grad. ``apply`` is called through ``mlp_block``, which decides ``save``: inside
    ``forward`` grad mode is always off and ``needs_input_grad`` ignores it. ``products`` is the library's code (products_code), 0 when left out; the
    backward runs with what the forward ran with."""

    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, eps, save, *products):
        x, w, b, gamma, beta = x.contiguous(), w.contiguous(), b.contiguous(), gamma.contiguous(), beta.contiguous()
        M, K = x.shape
        run = Launch(x)
        y = run.empty(M, HID)
        stats = run.empty(M, 2) if save else None
        code = products[0] if products else 0
        run("ac_mlp_block_forward_p", M, K, eps, x, w, b, gamma, beta, y, stats, code)
        if save:
            ctx.products, ctx.extra = code, len(products)
            ctx.save_for_backward(x, w, b, gamma, stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, b, gamma, stats = ctx.saved_tensors
        M, K = x.shape
        dy = dy.contiguous()
        run = Launch(x)
        ws = run.workspace("ac_mlp_block_workspace_floats", M, K)   # the partial sums
        dx = run.empty(M, K) if ctx.needs_input_grad[0] else None
        dw, db, dgamma, dbeta = run.empty(HID, K), run.empty(HID), run.empty(HID), run.empty(HID)
        run("ac_mlp_block_backward_p", M, K, dy, x, w, b, gamma, stats, ws, dx, dw, db, dgamma, dbeta, ctx.products)
        return (dx, dw, db, dgamma, dbeta, None, None) + (None,) * ctx.extra


def check_block(linear, act, norm, where="fc", device=True):
    """UnsupportedPolicy unless (linear, act, norm) is a block the kernels run: nn.Linear K -> 128 with bias and K <= 256, nn.ReLU,
    nn.LayerNorm(128) with affine parameters, float32; with ``device``, also on a CUDA device (checked at call time, so a policy can
    be swapped before it is moved). ``act`` None: the caller applies the kernel's ReLU whatever the module list says (mlp_block)."""
    bad = []
    if not isinstance(linear, nn.Linear):
        bad.append(f"not an nn.Linear ({type(linear).__name__})")
    else:
        if linear.out_features != HID:
            bad.append(f"out-features {linear.out_features} (only {HID})")
        if not 1 <= linear.in_features <= K_MAX:
            bad.append(f"in-features {linear.in_features} (at most {K_MAX})")
        bad += linear_faults(linear, device)
    if act is not None and not isinstance(act, nn.ReLU):
        bad.append(f"activation {type(act).__name__} (only ReLU, activation_id 1)")
    bad += layernorm_faults(norm, device)
    if bad:
        raise UnsupportedPolicy(f"{where}: " + ", ".join(bad))


def mlp_block(x, linear, norm, where="mlp_block", products="fp32"):
    """``norm(relu(linear(x)))`` as one fused kernel: x [..., K] float32 on the parameters' device -> [..., 128]. Something is saved
    for a backward only when grad mode is on and x or a parameter requires grad. ``products``: "fp32" or "bf16x3" (the module's
    docstring); anything else is a ValueError."""
    code = products_code(products)
    check_block(linear, None, norm, where)
    if x.dtype != torch.float32 or x.device != linear.weight.device:
        raise UnsupportedPolicy(f"{where}: input {x.dtype} on {x.device} (only float32 on {linear.weight.device})")
    if x.shape[-1] != linear.in_features:
        raise ValueError(f"{where}: input has {x.shape[-1]} features, the Linear takes {linear.in_features}")
    lead = x.shape[:-1]
    x2 = x.reshape(-1, linear.in_features)
    if x2.shape[0] == 0:
        return x.new_empty(lead + (HID,))
    args = (x2, linear.weight, linear.bias, norm.weight, norm.bias)
    save = torch.is_grad_enabled() and any(t.requires_grad for t in args)
    # "fp32" makes the call as it was before ``products`` existed, argument for argument (code 0 is forward's default)
    return DeviceMLPBlockFunction.apply(*args, float(norm.eps), save, *((code,) if code else ())).view(lead + (HID,))


def _triples(fc):
    return [(fc[j], fc[j + 1], fc[j + 2]) for j in range(0, len(fc), 3)]


def _fc_shaped(fc):
    return isinstance(fc, nn.Sequential) and len(fc) > 0 and len(fc) % 3 == 0 and \
        all(isinstance(l, nn.Linear) and isinstance(n, nn.LayerNorm) for l, _, n in _triples(fc))


def check_fc(fc, where="fc", device=True):
    if not _fc_shaped(fc):
        raise UnsupportedPolicy(f"{where}: not an nn.Sequential of (Linear, activation, LayerNorm) triples")
    for j, (lin, act, norm) in enumerate(_triples(fc)):
        check_block(lin, act, norm, f"{where}.{3 * j}", device)


class DeviceMLPLayer(nn.Module):
    """MLPLayer(input_dim, hidden_size, activation_id) of the reference with every block on the device: one child ``fc``
    (nn.Sequential of Linear, ReLU, LayerNorm triples), forward(x [..., input_dim]) -> [..., 128]. ``hidden_size`` is the reference's
    string of widths ("128 128"); only activation_id 1 (ReLU) is supported. Given ``fc``, that module is used as it is
    (use_device_mlp). ``products`` ("fp32" / "bf16x3") is kept as ``layer.products`` and given to every block."""

    def __init__(self, input_dim=HID, hidden_size="128 128", activation_id=1, fc=None, products="fp32"):
        products_code(products)
        super().__init__()
        self.products = products
        if fc is None:
            if activation_id != 1:
                raise UnsupportedPolicy(f"{type(self).__name__}: activation_id {activation_id} (only 1, ReLU)")
            size = [input_dim] + list(map(int, str(hidden_size).split(" ")))
            active = nn.ReLU()
            mods = []
            for j in range(len(size) - 1):
                mods += [nn.Linear(size[j], size[j + 1]), active, nn.LayerNorm(size[j + 1])]
            fc = nn.Sequential(*mods)
        check_fc(fc, type(self).__name__ + ".fc", device=False)
        self.fc = fc
        self._size = [fc[0].in_features] + [lin.out_features for lin, _, _ in _triples(fc)]
        self._hidden_layers = len(self._size) - 1

    def forward(self, x):
        for j, (lin, _, norm) in enumerate(_triples(self.fc)):
            x = mlp_block(x, lin, norm, f"{type(self).__name__}.fc.{3 * j}", self.products)
        return x

    @property
    def output_size(self):
        return self._size[-1]


def _mlp_layer_shaped(m):
    return not isinstance(m, DeviceMLPLayer) and _fc_shaped(getattr(m, "fc", None))


def use_device_mlp(module, products="fp32"):
    """Swap every MLPLayer-shaped module (one whose ``fc`` is an nn.Sequential of Linear, activation, LayerNorm triples) under
    ``module`` for a DeviceMLPLayer holding the very same ``fc``. ``module`` is an nn.Module (``policy.actor``, ``policy.critic``) or
    an object with ``actor`` / ``critic`` modules (the reference's PPO and MAPPO ``PPOPolicy``). Every layer is checked before any is
    swapped; an unsupported one raises UnsupportedPolicy naming it. Every swapped layer gets ``products`` ("fp32" / "bf16x3"; anything
    else is a ValueError before any module is touched). Returns the number of layers swapped."""
    products_code(products)
    return swap_children(module, _mlp_layer_shaped, lambda child, where: check_fc(child.fc, where + ".fc", device=False),
                         lambda child: DeviceMLPLayer(fc=child.fc, products=products), "an MLPLayer")
