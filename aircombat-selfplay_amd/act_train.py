"""The PPO / MAPPO update's action heads on the device ("The training action heads").

``ACTLayer.evaluate_actions`` of the reference (algorithms/utils/act.py) for MultiDiscrete spaces and the two tuple spaces with a shoot
part runs as one fused HIP kernel forward and two backward (csrc/act_train.hpp) on torch's current stream: every head's Linear,
log-softmax, taken entry and entropy, and the shoot head's Bernoulli, without logits or probabilities ever reaching memory; the backward
recomputes the logits and sums the parameter gradients in a fixed order.

``use_device_act(policy)`` makes the ``evaluate_actions`` of every ACTLayer-shaped module of a policy the device one. The module, its
children, state_dict, Parameter objects and ``forward`` (sampling) stay as they are, so optimiser state and checkpoints are unchanged.
It composes with ``use_device_gru`` and ``use_device_mlp`` in any order. The entropy's scaling, the loss and the optimiser stay torch.
"""
import ctypes as C
import types

import torch
import torch.nn as nn

from . import capi
from .policy import UnsupportedPolicy
from .train_common import Launch, linear_faults, policy_roots

HID = 128           # in-features of every head
MAX_CAT = 8         # categorical heads at most
MAX_LOGITS = 160    # their logits at most


def _ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class DeviceActEvalFunction(torch.autograd.Function):
    """(x [M, 128], action [M, n_cat + n_shoot_cols], alpha0, beta0 [M] or None, nvec, n_shoot_cols, save, W_0, b_0, W_1, b_1, ...) ->
    (logp [M], ent [M]): the sum over heads of the taken action's log-probability and of the entropy, unscaled. The parameters are the
    categorical heads' in order and then, with shoot columns, the one shoot head's. With ``save`` the inputs are kept and the backward
    recomputes the logits from them; ``dx`` is computed only when ``x`` requires grad. ``apply`` is called through ``act_evaluate``,
    which decides ``save``: inside ``forward`` grad mode is always off and ``needs_input_grad`` ignores it."""

    @staticmethod
    def forward(ctx, x, action, alpha0, beta0, nvec, n_shoot_cols, save, *params):
        heads = capi.AcActHeads(n_cat=len(nvec), n_shoot_cols=n_shoot_cols)
        heads.nvec[:len(nvec)] = list(nvec)
        params = tuple(p.contiguous() for p in params)
        M = x.shape[0]
        run = Launch(x)
        logp, ent = run.empty(M), run.empty(M)
        run("ac_act_eval_forward", C.byref(heads), M, x, _ptrs(params[0::2]), _ptrs(params[1::2]), action, alpha0, beta0, logp, ent)
        if save:
            ctx.heads, ctx.shoot = heads, alpha0 is not None
            ctx.set_materialize_grads(False)   # an unused output's gradient arrives as None and goes to the kernel as NULL
            ctx.save_for_backward(x, action, *(() if alpha0 is None else (alpha0, beta0)), *params)
        return logp, ent

    @staticmethod
    def backward(ctx, dlogp, dent):
        x, action, *rest = ctx.saved_tensors
        alpha0, beta0 = (rest[0], rest[1]) if ctx.shoot else (None, None)
        params = rest[2:] if ctx.shoot else rest
        M = x.shape[0]
        dlogp = None if dlogp is None else dlogp.contiguous()
        dent = None if dent is None else dent.contiguous()
        run = Launch(x)
        ws = run.workspace("ac_act_eval_workspace_floats", C.byref(ctx.heads), M)   # the partial sums
        dx = run.empty(M, HID) if ctx.needs_input_grad[0] else None
        grads = [torch.empty_like(p) for p in params]
        run("ac_act_eval_backward", C.byref(ctx.heads), M, dlogp, dent, x, _ptrs(params[0::2]), _ptrs(params[1::2]), action, alpha0, beta0, ws,
            dx, _ptrs(grads[0::2]), _ptrs(grads[1::2]))
        return (dx, None, None, None, None, None, None, *grads)


def _split(action_outs):
    """(categorical heads, shoot heads) of an ACTLayer's ``action_outs``, or None if it is not that shape: leading members with a
    ``logits_net``, then trailing members with a ``net``, nothing else."""
    if not isinstance(action_outs, nn.ModuleList):
        return None
    mods = list(action_outs)
    n_cat = 0
    while n_cat < len(mods) and isinstance(getattr(mods[n_cat], "logits_net", None), nn.Module):
        n_cat += 1
    cats, shoots = mods[:n_cat], mods[n_cat:]
    if not all(isinstance(getattr(m, "net", None), nn.Module) and not hasattr(m, "logits_net") for m in shoots):
        return None
    return cats, shoots


def check_heads(action_outs, where="action_outs", device=True):
    """UnsupportedPolicy unless ``action_outs`` is what the kernels run: 1 .. 8 heads ``logits_net = nn.Linear(128, n >= 2)`` with at
    most 160 logits in all, then 0, 1 or 4 heads ``net = nn.Linear(128, 2)``, every Linear with bias and float32; with ``device``, also
    on a CUDA device (checked at call time, so a policy can be swapped before it is moved). Returns (the Linear modules that take
    part: the categorical heads' and, with shoot heads, the LAST one's; nvec; the number of shoot columns)."""
    parts = _split(action_outs)
    if parts is None:
        raise UnsupportedPolicy(f"{where}: not an nn.ModuleList of logits_net heads followed by net (shoot) heads")
    cats, shoots = parts
    bad = []
    if not 1 <= len(cats) <= MAX_CAT:
        bad.append(f"{len(cats)} categorical heads (1 .. {MAX_CAT})")
    if len(shoots) not in (0, 1, 4):
        bad.append(f"{len(shoots)} trailing shoot heads (only 0, 1 or 4)")
    linears = [m.logits_net for m in cats] + [m.net for m in shoots]
    for i, lin in enumerate(linears):
        at = f"{where}.{i}.{'logits_net' if i < len(cats) else 'net'}"
        if not isinstance(lin, nn.Linear):
            bad.append(f"{at} is not an nn.Linear ({type(lin).__name__})")
            continue
        if lin.in_features != HID:
            bad.append(f"{at}: in-features {lin.in_features} (only {HID})")
        if i < len(cats) and lin.out_features < 2:
            bad.append(f"{at}: {lin.out_features} logits (at least 2)")
        if i >= len(cats) and lin.out_features != 2:
            bad.append(f"{at}: out-features {lin.out_features} (only 2)")
        bad += [f"{at}: {fault}" for fault in linear_faults(lin, device)]
    nvec = [lin.out_features for lin in linears[:len(cats)] if isinstance(lin, nn.Linear)]
    if sum(nvec) > MAX_LOGITS:
        bad.append(f"{sum(nvec)} logits (at most {MAX_LOGITS})")
    if bad:
        raise UnsupportedPolicy(f"{where}: " + ", ".join(bad))
    return linears[:len(cats)] + linears[-1:] * bool(shoots), nvec, len(shoots)


def act_evaluate(x, action_outs, action, active_masks=None, where="action_outs", **kwargs):
    """``ACTLayer.evaluate_actions`` after its optional MLP, over the ``action_outs`` of a MultiDiscrete or tuple (shoot) space:
    x [M, 128] float32 on the parameters' CUDA device, action [M, n_cat + n_shoot_cols] -> (action_log_probs [M, 1], dist_entropy
    [M, 1]). As in the reference only the LAST shoot head is evaluated, on all the shoot columns, and its entropy is counted once; a
    tuple space needs the ``alpha0=`` / ``beta0=`` tensors [M, 1] (KeyError without them). Something is saved for a backward only when
    grad mode is on and x or a parameter requires grad."""
    linears, nvec, n_shoot = check_heads(action_outs, where)
    dev = linears[0].weight.device
    if x.dtype != torch.float32 or x.device != dev:
        raise UnsupportedPolicy(f"{where}: input {x.dtype} on {x.device} (only float32 on {dev})")
    if x.dim() != 2 or x.shape[1] != HID:
        raise ValueError(f"{where}: input of shape {tuple(x.shape)}, the heads take [M, {HID}]")
    M, cols = x.shape[0], len(nvec) + n_shoot
    if tuple(action.shape) != (M, cols):
        raise ValueError(f"{where}: action of shape {tuple(action.shape)}, expected {(M, cols)}")
    prior = lambda t: t.to(device=dev, dtype=torch.float32).reshape(M).contiguous()
    alpha0, beta0 = (prior(kwargs["alpha0"]), prior(kwargs["beta0"])) if n_shoot else (None, None)
    action = action.to(device=dev, dtype=torch.float32).contiguous()
    params = [p for lin in linears for p in (lin.weight, lin.bias)]
    if M == 0:
        logp = ent = x.new_zeros(0)
    else:
        x = x.contiguous()
        save = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        logp, ent = DeviceActEvalFunction.apply(x, action, alpha0, beta0, tuple(nvec), n_shoot, save, *params)
    logp, ent = logp.view(M, 1), ent.view(M, 1)
    if active_masks is not None:
        return logp, ent * active_masks / active_masks.sum()
    return logp, ent / M


def _device_evaluate_actions(self, x, action, active_masks=None, **kwargs):
    """ACTLayer.evaluate_actions with the heads on the device (use_device_act)."""
    if getattr(self, "_mlp_actlayer", isinstance(getattr(self, "mlp", None), nn.Module)):
        x = self.mlp(x)
    return act_evaluate(x, self.action_outs, action, active_masks, where=type(self).__name__ + ".action_outs", **kwargs)


def _act_layer_shaped(m):
    return isinstance(getattr(m, "action_outs", None), nn.ModuleList) or isinstance(getattr(m, "action_out", None), nn.Module)


def _swapped(m):
    return getattr(m.__dict__.get("evaluate_actions"), "__func__", None) is _device_evaluate_actions


def use_device_act(module):
    """Make ``evaluate_actions`` of every ACTLayer-shaped module (one with an nn.ModuleList ``action_outs`` of ``logits_net`` heads and
    0, 1 or 4 trailing ``net`` heads) under ``module`` the device one. ``module`` is an nn.Module (``policy.actor``) or an object with
    ``actor`` / ``critic`` modules (the reference's PPO and MAPPO ``PPOPolicy``). The module object, its children, state_dict,
    Parameter objects and ``forward`` stay as they are; ``copy.deepcopy`` of it runs the device path too. Every layer is checked before
    any is changed; an unsupported one (a single ``action_out``: Discrete, Box, MultiBinary) raises UnsupportedPolicy naming it.
    Returns the number of layers changed."""
    found = []
    for root, prefix in policy_roots(module):
        for name, m in root.named_modules():
            if _act_layer_shaped(m) and not _swapped(m):
                found.append((m, prefix + name if name else (prefix.rstrip(".") or type(root).__name__)))
    for m, where in found:
        if not isinstance(getattr(m, "action_outs", None), nn.ModuleList):
            raise UnsupportedPolicy(f"{where}.action_out: a single {type(m.action_out).__name__} head (Discrete, Box or MultiBinary space); "
                                    "only MultiDiscrete and the tuple spaces with a shoot part")
        check_heads(m.action_outs, where + ".action_outs", device=False)
    for m, _ in found:
        m.evaluate_actions = types.MethodType(_device_evaluate_actions, m)   # (a bound method in __dict__: deepcopy rebinds it to the copy)
    return len(found)
