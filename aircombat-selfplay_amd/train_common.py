"""What the device training layers share on the Python side (gru_train, gru_layer_train, mlp_train, act_train, ppo_update; DESIGN.md §5,
"What the training layers share"): the launch helper every autograd body calls the library through, the walker behind the
``use_device_*`` functions, and the faults of the two torch modules more than one layer checks. ``csrc/train_common.hpp`` is the
library's half.
"""
import torch
import torch.nn as nn

from . import capi
from .policy import UnsupportedPolicy

HID = 128   # the width of every LayerNorm the kernels run
PRODUCTS = {"fp32": 0, "bf16x3": 1}   # AC_PRODUCTS_FP32, AC_PRODUCTS_BF16X3 (include/aircombat.h)


def products_code(value, name="products"):
    """The library's constant for ``value``, the argument called ``name`` ("products" or "dense_products"); ValueError for anything but
    "fp32" / "bf16x3"."""
    if not isinstance(value, str) or value not in PRODUCTS:
        raise ValueError(f"{name} must be one of {', '.join(map(repr, PRODUCTS))}, not {value!r}")
    return PRODUCTS[value]


class Launch:
    """The library, the device and torch's current stream there, from the tensor ``x`` that decides the device. One per autograd body:
    the stream is read once, when it is built."""
    __slots__ = ("lib", "dev", "stream")

    def __init__(self, x):
        self.lib = capi.load_library()
        self.dev = dev = x.device
        # torch.cuda.current_stream(dev).cuda_stream without the Stream object in between (1.9 us against 0.1 us, on every launch of an
        # update that is host-bound at small batches); torch's own generated code reads the stream the same way. A CPU tensor has no
        # device index and no stream: only workspace()'s refusals can be reached with one.
        self.stream = torch._C._cuda_getCurrentRawStream(dev.index) if dev.index is not None else None

    def empty(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.dev)

    def workspace(self, symbol, *args):
        """The workspace ``symbol`` (a ``*_workspace_floats``) sizes for ``args``, as a tensor: torch's allocator orders its reuse on
        the stream. A shape the library refuses is its RuntimeError, not a torch size error."""
        floats = getattr(self.lib, symbol)(*args)
        if floats < 0:
            raise RuntimeError(f"{symbol} failed: {self.lib.last_error()}")
        return self.empty(floats)

    def __call__(self, symbol, *args):
        """``symbol(device index, stream, *args)`` with every tensor among ``args`` as its ``data_ptr()`` and anything else (None,
        numbers, ctypes values) as given; RuntimeError with the library's message unless it returns 0. The caller keeps the tensors
        (a ``contiguous()`` result too) alive in locals until this returns."""
        rc = getattr(self.lib, symbol)(self.dev.index, self.stream, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])
        self.lib.check(rc, symbol)


def policy_roots(module):
    """The (root module, prefix of its names) pairs of ``module``: an nn.Module itself, or the ``actor`` / ``critic`` modules of an
    object holding them (the reference's PPO and MAPPO ``PPOPolicy``)."""
    roots = [(module, "")] if isinstance(module, nn.Module) else \
        [(getattr(module, k), k + ".") for k in ("actor", "critic") if isinstance(getattr(module, k, None), nn.Module)]
    if not roots:
        raise UnsupportedPolicy(f"{type(module).__name__}: neither an nn.Module nor an object with actor / critic modules")
    return roots


def swap_children(module, shaped, check, build, itself):
    """Replace every child under ``module`` that ``shaped(child)`` accepts with ``build(child)``. ``check(child, where)`` raises
    UnsupportedPolicy for a child that cannot be run, ``where`` being its dotted name; every child is checked before any is replaced. A
    root that is itself such a layer (``itself``: "a GRULayer") has no parent to replace it in and is refused. Returns the number
    replaced."""
    found = []
    for root, prefix in policy_roots(module):
        if shaped(root):
            raise UnsupportedPolicy(f"{prefix or type(root).__name__}: {itself} itself cannot be swapped in place; pass the module holding it")
        for pname, parent in root.named_modules():
            for cname, child in parent.named_children():
                if shaped(child):
                    found.append((parent, cname, child, prefix + (pname + "." if pname else "") + cname))
    for _, _, child, where in found:
        check(child, where)
    for parent, cname, child, _ in found:
        setattr(parent, cname, build(child))
    return len(found)


def layernorm_faults(norm, device=True):
    """What keeps ``norm`` from being the kernels' LayerNorm, as a list of strings (empty: nothing): nn.LayerNorm((128,)) with affine
    parameters, float32 and, with ``device``, on a CUDA device."""
    if not isinstance(norm, nn.LayerNorm):
        return [f"not an nn.LayerNorm ({type(norm).__name__})"]
    bad = []
    if tuple(norm.normalized_shape) != (HID,):
        bad.append(f"LayerNorm over {tuple(norm.normalized_shape)} (only ({HID},))")
    if norm.weight is None or norm.bias is None:
        bad.append("LayerNorm without affine parameters")
    elif norm.weight.dtype != torch.float32:
        bad.append(f"LayerNorm dtype {norm.weight.dtype} (only float32)")
    elif device and norm.weight.device.type != "cuda":
        bad.append(f"LayerNorm device {norm.weight.device} (only a CUDA device)")
    return bad


def linear_faults(linear, device=True):
    """What keeps the nn.Linear ``linear`` from being one the kernels read, whatever its sizes: with bias, float32 and, with ``device``,
    on a CUDA device."""
    bad = []
    if linear.bias is None:
        bad.append("Linear without bias")
    if linear.weight.dtype != torch.float32:
        bad.append(f"dtype {linear.weight.dtype} (only float32)")
    if device and linear.weight.device.type != "cuda":
        bad.append(f"device {linear.weight.device} (only a CUDA device)")
    return bad
