"""The PPO / MAPPO update's actor and critic as one device call each ("The networks as one call").

``use_device_mlp``, ``use_device_gru_layer`` and ``use_device_act`` give every layer of ``evaluate_actions`` a fused kernel, but Python
and autograd still glue them: one ``autograd.Function`` per layer, five in each network, forward and again backward. At the reference's
minibatch shapes that glue, not the kernels, sets the time. Here a whole network is ONE ``autograd.Function`` and one C call per
direction (csrc/net_train.hpp), which queues the very same layer launches back to back on torch's current stream; autograd still joins
actor, critic and loss. Three small kernels fill what was still eager torch:

``value_head(x, linear)``      the critic's ``value_out``;
``feature_norm(x, norm)``      the optional ``base.feature_norm`` over the raw observation;
``shoot_prior(obs)``           ``alpha0`` / ``beta0`` of ``use_prior`` (algorithms/ppo/ppo_actor.py:40-49), not differentiable.

``use_device_networks(policy)`` makes ``actor.evaluate_actions`` and ``critic.forward`` the device methods by binding them in the
instance ``__dict__`` (as ``use_device_act`` does): module objects, Parameters, ``state_dict`` keys and the optimiser stay as they are,
and it works whether or not the per-layer swaps were applied before. Results are those of the layered path bit for bit.
"""
import ctypes as C
import types
import weakref

import numpy as np
import torch
import torch.nn as nn

from . import capi
from .act_train import check_heads
from .gru_layer_train import check_layer, dense_products_code
from .mlp_train import K_MAX, _triples, check_fc
from .policy import UnsupportedPolicy
from .train_common import HID, Launch, linear_faults, policy_roots, products_code

MAX_BLOCKS = capi.AC_NET_MAX_BLOCKS
PRIOR_COLUMNS = 14   # the prior reads columns 11 and 13 of the observation


def constants():
    """The three kernels' constants: rows per tile, the forwards' workgroups at most, the backwards' (their partial sets at most)."""
    lib = capi.load_library()
    return {k: lib.ac_net_constant(i) for i, k in enumerate(("rows", "forward_workgroups", "backward_workgroups"))}


# ---------------------------------------------------------------------------------------------------------------- the three pieces
class DeviceValueHeadFunction(torch.autograd.Function):
    """(x [M, 128], w [1, 128], b [1], save) -> v [M] = x wᵀ + b. With ``save`` x and w are kept; ``dx`` is computed only when x requires
    grad. ``apply`` is called through ``value_head``, which decides ``save``."""

    @staticmethod
    def forward(ctx, x, w, b, save):
        x, w, b = x.contiguous(), w.contiguous(), b.contiguous()
        M = x.shape[0]
        run = Launch(x)
        v = run.empty(M)
        run("ac_value_head_forward", M, x, w, b, v)
        if save:
            ctx.save_for_backward(x, w)
        return v

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        M = x.shape[0]
        g = g.contiguous()
        run = Launch(x)
        ws = run.workspace("ac_value_head_workspace_floats", M)   # the partial sums
        dx = run.empty(M, HID) if ctx.needs_input_grad[0] else None
        dw, db = run.empty(1, HID), run.empty(1)
        run("ac_value_head_backward", M, g, x, w, ws, dx, dw, db)
        return dx, dw, db, None


def value_out_faults(linear, device=True):
    """What keeps ``linear`` from being the critic's value head, as a list of strings: nn.Linear(128, 1) with bias, float32 and, with
    ``device``, on a CUDA device."""
    if not isinstance(linear, nn.Linear):
        return [f"not an nn.Linear ({type(linear).__name__})"]
    bad = []
    if (linear.in_features, linear.out_features) != (HID, 1):
        bad.append(f"Linear({linear.in_features}, {linear.out_features}) (only Linear({HID}, 1))")
    return bad + linear_faults(linear, device)


def feature_norm_faults(norm, width=None, device=True):
    """What keeps ``norm`` from being the kernels' feature norm: nn.LayerNorm over one axis of 1 .. 256 entries (``width``, when given:
    exactly that many), with affine parameters, float32 and, with ``device``, on a CUDA device."""
    if not isinstance(norm, nn.LayerNorm):
        return [f"not an nn.LayerNorm ({type(norm).__name__})"]
    bad = []
    shape = tuple(norm.normalized_shape)
    if len(shape) != 1 or not 1 <= shape[0] <= K_MAX:
        bad.append(f"LayerNorm over {shape} (one axis of at most {K_MAX})")
    elif width is not None and shape[0] != width:
        bad.append(f"LayerNorm over {shape} (the input's width is {width})")
    if norm.weight is None or norm.bias is None:
        bad.append("LayerNorm without affine parameters")
    elif norm.weight.dtype != torch.float32:
        bad.append(f"LayerNorm dtype {norm.weight.dtype} (only float32)")
    elif device and norm.weight.device.type != "cuda":
        bad.append(f"LayerNorm device {norm.weight.device} (only a CUDA device)")
    return bad


def _input_ok(x, param, width, where):
    if x.dtype != torch.float32 or x.device != param.device:
        raise UnsupportedPolicy(f"{where}: input {x.dtype} on {x.device} (only float32 on {param.device})")
    if x.dim() < 1 or x.shape[-1] != width:
        raise ValueError(f"{where}: input of shape {tuple(x.shape)}, expected [..., {width}]")


def value_head(x, linear, where="value_head"):
    """``linear(x)`` for the critic's ``value_out = nn.Linear(128, 1)`` as one kernel: x [..., 128] float32 on the parameters' CUDA
    device -> [..., 1]. Something is saved for a backward only when grad mode is on and x or a parameter requires grad."""
    bad = value_out_faults(linear)
    if bad:
        raise UnsupportedPolicy(f"{where}: " + ", ".join(bad))
    _input_ok(x, linear.weight, HID, where)
    lead = x.shape[:-1]
    x2 = x.reshape(-1, HID)
    if x2.shape[0] == 0:
        return x.new_empty(lead + (1,))
    save = torch.is_grad_enabled() and (x2.requires_grad or linear.weight.requires_grad or linear.bias.requires_grad)
    return DeviceValueHeadFunction.apply(x2, linear.weight, linear.bias, save).view(lead + (1,))


class DeviceFeatureNormFunction(torch.autograd.Function):
    """(x [M, K], gamma, beta [K], eps, save) -> y [M, K] = LayerNorm_K(x) * gamma + beta, biased variance. With ``save`` the forward keeps
    each row's mean and 1/std (8 bytes per row), as the MLP block keeps its ``stats``; ``dx`` is computed only when x requires grad.
    ``apply`` is called through ``feature_norm``, which decides ``save``."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, save):
        x, gamma, beta = x.contiguous(), gamma.contiguous(), beta.contiguous()
        M, K = x.shape
        run = Launch(x)
        y = run.empty(M, K)
        stats = run.empty(M, 2) if save else None
        run("ac_feature_norm_forward", M, K, eps, x, gamma, beta, y, stats)
        if save:
            ctx.save_for_backward(x, gamma, stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, stats = ctx.saved_tensors
        M, K = x.shape
        dy = dy.contiguous()
        run = Launch(x)
        ws = run.workspace("ac_feature_norm_workspace_floats", M, K)   # the partial sums
        dx = run.empty(M, K) if ctx.needs_input_grad[0] else None
        dgamma, dbeta = run.empty(K), run.empty(K)
        run("ac_feature_norm_backward", M, K, dy, x, gamma, stats, ws, dx, dgamma, dbeta)
        return dx, dgamma, dbeta, None, None


def feature_norm(x, norm, where="feature_norm"):
    """``norm(x)`` for ``base.feature_norm = nn.LayerNorm(K)``, K <= 256, as one kernel: x [..., K] float32 on the parameters' CUDA
    device -> [..., K]. Something is saved for a backward only when grad mode is on and x or a parameter requires grad."""
    bad = feature_norm_faults(norm)
    if bad:
        raise UnsupportedPolicy(f"{where}: " + ", ".join(bad))
    K = norm.normalized_shape[0]
    _input_ok(x, norm.weight, K, where)
    x2 = x.reshape(-1, K)
    if x2.shape[0] == 0:
        return x.new_empty(x.shape)
    save = torch.is_grad_enabled() and (x2.requires_grad or norm.weight.requires_grad or norm.bias.requires_grad)
    return DeviceFeatureNormFunction.apply(x2, norm.weight, norm.bias, float(norm.eps), save).view(x.shape)


def shoot_prior(obs):
    """(alpha0, beta0), each [M, 1], of the reference actor's ``use_prior`` from obs [M, K >= 14] float32 on a CUDA device: alpha0 is 10 /
    6 / 3 as ``obs[:, 13] * 10000`` is <= 8000, <= 12000 or neither, beta0 3 / 6 / 10 as ``rad2deg(obs[:, 11])`` is <= 22.5, <= 45 or
    neither, in the reference's fp32 arithmetic. Not differentiable."""
    if not isinstance(obs, torch.Tensor) or obs.dtype != torch.float32 or obs.device.type != "cuda":
        what = f"{obs.dtype} on {obs.device}" if isinstance(obs, torch.Tensor) else type(obs).__name__
        raise UnsupportedPolicy(f"shoot_prior: obs is {what} (only float32 on a CUDA device)")
    if obs.dim() != 2 or obs.shape[1] < PRIOR_COLUMNS:
        raise ValueError(f"shoot_prior: obs of shape {tuple(obs.shape)}, expected [M, K >= {PRIOR_COLUMNS}]")
    obs = obs.detach().contiguous()
    M, K = obs.shape
    run = Launch(obs)
    alpha0, beta0 = run.empty(M, 1), run.empty(M, 1)
    if M:
        run("ac_shoot_prior", M, K, obs, alpha0, beta0)
    return alpha0, beta0


# ---------------------------------------------------------------------------------------------------------------- a whole network
def _ptr_table(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class NetCall:
    """What one call of a network function needs besides its tensors: the packed ``ac_net_t`` (its parameter pointers are filled by the
    forward), the chunk count N, the chunk length T and ``save``, decided outside ``forward``."""
    __slots__ = ("net", "N", "T", "save", "sizes")

    def __init__(self, net, N, T, save, sizes):
        self.net, self.N, self.T, self.save, self.sizes = net, N, T, save, sizes

    def floats(self, run):
        """(workspace floats, saved floats) for this shape, asked of the library once per shape."""
        key = (self.N, self.T)
        if key not in self.sizes:
            got = []
            for symbol in ("ac_net_workspace_floats", "ac_net_saved_floats"):
                n = getattr(run.lib, symbol)(C.byref(self.net), self.N, self.T)
                if n < 0:
                    raise RuntimeError(f"{symbol} failed: {run.lib.last_error()}")
                got.append(n)
            self.sizes[key] = tuple(got)
        return self.sizes[key]


def _net_forward(ctx, symbol, tensors, params, call, outs):
    run = Launch(tensors[0])
    net = call.net
    for i, p in enumerate(params):
        net.params[i] = p.data_ptr()
    ws_floats, saved_floats = call.floats(run)
    # workspace and saved activations are torch tensors: torch's allocator orders their reuse on this stream
    ws = run.empty(ws_floats)
    saved = run.empty(saved_floats) if call.save else None
    outs = [run.empty(*shape(call)) for shape in outs]
    run(symbol, C.byref(net), call.N, call.T, *tensors, ws, saved, *outs)
    if call.save:
        ctx.call, ctx.n_in = call, len(tensors)
        ctx.save_for_backward(*tensors, saved, *params)
    ctx.set_materialize_grads(False)   # an unused output's gradient arrives as None and goes to the library as NULL
    return tuple(outs)


def _net_backward(ctx, symbol, g0, g1):
    call, n_in = ctx.call, ctx.n_in
    tensors, saved, params = ctx.saved_tensors[:n_in], ctx.saved_tensors[n_in], ctx.saved_tensors[n_in + 1:]
    run = Launch(saved)
    net = call.net
    for i, p in enumerate(params):   # (another forward of the same network may have run in between)
        net.params[i] = p.data_ptr()
    ws = run.empty(call.floats(run)[0])
    grads = [torch.empty_like(p) for p in params]
    g0 = None if g0 is None else g0.contiguous()
    g1 = None if g1 is None else g1.contiguous()
    run(symbol, C.byref(net), call.N, call.T, g0, g1, *tensors, saved, ws, _ptr_table(grads))
    return (None,) * n_in + tuple(grads) + (None,)


class DeviceActorEvalFunction(torch.autograd.Function):
    """(obs [T*N, K], rnn_states [N, 128], masks [T*N], action [T*N, columns], the parameters in ``ac_net_t``'s order, a NetCall) ->
    (logp [M], ent [M]), unscaled as ``DeviceActEvalFunction``'s: the reference actor's ``evaluate_actions`` as one C call forward and
    one backward. obs, rnn_states, masks and action take no gradient. ``apply`` is called through the method ``use_device_networks``
    binds, which decides ``NetCall.save``: inside ``forward`` grad mode is always off and ``needs_input_grad`` ignores it."""

    @staticmethod
    def forward(ctx, obs, rnn_states, masks, action, *rest):
        M = lambda call: (call.N * call.T,)
        return _net_forward(ctx, "ac_actor_eval_forward", (obs, rnn_states, masks, action), rest[:-1], rest[-1], (M, M))

    @staticmethod
    def backward(ctx, dlogp, dent):
        return _net_backward(ctx, "ac_actor_eval_backward", dlogp, dent)


class DeviceCriticFunction(torch.autograd.Function):
    """(obs [T*N, K], rnn_states [N, 128], masks [T*N], the parameters in ``ac_net_t``'s order, a NetCall) -> (values [M, 1],
    h_T [N, 128]): the reference critic's ``forward`` as one C call forward and one backward. obs, rnn_states and masks take no
    gradient."""

    @staticmethod
    def forward(ctx, obs, rnn_states, masks, *rest):
        return _net_forward(ctx, "ac_critic_forward", (obs, rnn_states, masks), rest[:-1], rest[-1],
                            (lambda call: (call.N * call.T, 1), lambda call: (call.N, HID)))

    @staticmethod
    def backward(ctx, dvalues, dh_T):
        if dvalues is None:   # only h_T was used: value_out and the head blocks get zero gradients, not None
            dvalues = torch.zeros(ctx.call.N * ctx.call.T, dtype=torch.float32, device=ctx.saved_tensors[0].device)
        return _net_backward(ctx, "ac_critic_backward", dvalues, dh_T)


class NetDescription:
    """One network as ``use_device_networks`` reads it: ``kind`` ("actor" / "critic"), the parameters in ``ac_net_t``'s order and the
    struct's other fields. ``describe`` builds it, or raises UnsupportedPolicy naming the module that cannot be run."""
    __slots__ = ("kind", "params", "obs_dim", "feature_norm", "base_blocks", "head_blocks", "nvec", "n_shoot", "eps")

    def pack(self, mlp_products="fp32", products="fp32", dense_products="fp32"):
        """The ``ac_net_t`` (capi.AcNet) of this description with the three product choices; the parameter pointers stay NULL."""
        net = capi.AcNet(obs_dim=self.obs_dim, feature_norm=int(self.feature_norm), base_blocks=self.base_blocks, head_blocks=self.head_blocks,
                         mlp_products=products_code(mlp_products, "mlp_products"), gru_products=products_code(products),
                         gru_dense_products=dense_products_code(dense_products))
        net.heads.n_cat, net.heads.n_shoot_cols = len(self.nvec), self.n_shoot
        net.heads.nvec[:len(self.nvec)] = list(self.nvec)
        net.feature_norm_eps, net.gru_eps = self.eps["feature_norm"], self.eps["gru"]
        net.block_eps[:len(self.eps["blocks"])] = self.eps["blocks"]
        return net


def _kind(root):
    if isinstance(getattr(root, "act", None), nn.Module):
        return "actor"
    if hasattr(root, "value_out"):
        return "critic"
    return None


def _head_mlp(holder):
    """The head MLP of ``holder`` (the actor's ``act``, or the critic), or None when it has none (an empty ``act_hidden_size``)."""
    mlp = getattr(holder, "mlp", None)
    return mlp if getattr(holder, "_mlp_actlayer", isinstance(mlp, nn.Module)) else None


def describe(root, prefix="", device=True):
    """The NetDescription of ``root`` (an actor: it has ``act``; or a critic: it has ``value_out``), reading the children
    ``base.feature_norm``, ``base.mlp.fc``, ``rnn.gru``, ``rnn.norm``, ``act.mlp.fc``, ``act.action_outs`` or ``mlp.fc``, ``value_out``.
    Everything that keeps it from running is collected and raised as one UnsupportedPolicy, each fault behind its module path
    (``prefix`` in front); with ``device`` False the parameters need not be on a CUDA device yet."""
    kind = _kind(root)
    if kind is None:
        raise UnsupportedPolicy(f"{prefix or type(root).__name__}: neither an actor (no act module) nor a critic (no value_out)")
    said, d = [], NetDescription()
    d.kind, d.nvec, d.n_shoot, d.eps = kind, (), 0, {"feature_norm": 1e-5, "gru": 1e-5, "blocks": []}

    def attempt(check, *args):
        try:
            return check(*args)
        except UnsupportedPolicy as exc:
            said.append(str(exc))
            return None

    def blocks(fc, where):
        """The parameters of an MLPLayer's ``fc``; its blocks' eps are noted."""
        faults = len(said)
        attempt(check_fc, fc, where, device)
        if len(said) > faults:
            return [], 0
        triples = _triples(fc)
        if len(triples) > MAX_BLOCKS:
            said.append(f"{where}: {len(triples)} blocks (at most {MAX_BLOCKS})")
        d.eps["blocks"] += [float(norm.eps) for _, _, norm in triples]
        return [p for lin, _, norm in triples for p in (lin.weight, lin.bias, norm.weight, norm.bias)], len(triples)

    params = []
    base = getattr(root, "base", None)
    fc = getattr(getattr(base, "mlp", None), "fc", None)
    got, d.base_blocks = blocks(fc, f"{prefix}base.mlp.fc")
    d.obs_dim = fc[0].in_features if d.base_blocks else 0
    norm = getattr(base, "feature_norm", None) if getattr(base, "_use_feature_normalization", True) else None
    d.feature_norm = norm is not None
    if d.feature_norm:
        bad = feature_norm_faults(norm, d.obs_dim or None, device)
        if bad:
            said.append(f"{prefix}base.feature_norm: " + ", ".join(bad))
        else:
            params += [norm.weight, norm.bias]
            d.eps["feature_norm"] = float(norm.eps)
    params += got
    rnn = getattr(root, "rnn", None)
    if not getattr(root, "use_recurrent_policy", True) or rnn is None:
        said.append(f"{prefix}rnn: use_recurrent_policy=False (the networks run with their GRU layer only)")
    else:
        faults = len(said)
        attempt(check_layer, getattr(rnn, "gru", None), getattr(rnn, "norm", None), f"{prefix}rnn", device)
        if getattr(rnn, "_num_layers", 1) != 1:
            said.append(f"{prefix}rnn: {rnn._num_layers} layers (only 1)")
        if len(said) == faults:
            g = rnn.gru
            params += [g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0, rnn.norm.weight, rnn.norm.bias]
            d.eps["gru"] = float(rnn.norm.eps)
    holder, hname = (root.act, f"{prefix}act.") if kind == "actor" else (root, prefix)
    mlp = _head_mlp(holder)
    d.head_blocks = 0
    if mlp is not None:
        got, d.head_blocks = blocks(getattr(mlp, "fc", None), f"{hname}mlp.fc")
        params += got
    if kind == "actor":
        outs = getattr(holder, "action_outs", None)
        if not isinstance(outs, nn.ModuleList):
            single = getattr(holder, "action_out", None)
            said.append(f"{hname}action_out: a single {type(single).__name__} head (Discrete, Box or MultiBinary space); only MultiDiscrete "
                        "and the tuple spaces with a shoot part")
        else:
            got = attempt(check_heads, outs, f"{hname}action_outs", device)
            if got is not None:
                linears, nvec, d.n_shoot = got
                d.nvec = tuple(nvec)
                params += [p for lin in linears for p in (lin.weight, lin.bias)]
                prior = bool(getattr(root, "use_prior", False))
                if d.n_shoot and not prior:
                    said.append(f"{hname}action_outs: shoot heads without use_prior (the reference gives them no alpha0 / beta0)")
                if d.n_shoot and 0 < d.obs_dim < PRIOR_COLUMNS:
                    said.append(f"{prefix}base.mlp.fc.0: in-features {d.obs_dim} (the shoot prior reads columns 11 and 13)")
    else:
        bad = value_out_faults(root.value_out, device)
        if bad:
            said.append(f"{prefix}value_out: " + ", ".join(bad))
        else:
            params += [root.value_out.weight, root.value_out.bias]
    if said:
        raise UnsupportedPolicy("; ".join(said))
    d.params = tuple(params)
    return d


class _Plan:
    """A patched network's description, packed once per (module, product choice) and kept outside the module (a ctypes struct does not
    deepcopy): a copy of the module builds its own at its first call, from its own parameters. ``links`` is what the description was
    read through: every (``_modules`` or ``_parameters`` dict, key, object found there) on the way from the network to each of its
    parameters. A call whose links no longer hold (a Parameter or a child module was replaced) reads the network again."""
    __slots__ = ("desc", "net", "sizes", "choice", "links")

    def holds(self):
        for holder, key, found in self.links:
            if holder.get(key) is not found:
                return False
        return True


_PLANS = weakref.WeakKeyDictionary()


def _links(module, params):
    """The links of ``params`` under ``module`` (_Plan), each once."""
    names = {id(p): name for name, p in module.named_parameters(remove_duplicate=False)}
    links, seen = [], set()
    for p in params:
        at, path = module, names[id(p)].split(".")
        for i, key in enumerate(path):
            holder = at._parameters if i == len(path) - 1 else at._modules
            if (id(holder), key) not in seen:
                seen.add((id(holder), key))
                links.append((holder, key, holder[key]))
            at = holder[key]
    return tuple(links)


def _plan(module):
    choice = tuple(module._device_net[k] for k in ("mlp_products", "products", "dense_products"))
    plan = _PLANS.get(module)
    if plan is None or plan.choice != choice or not plan.holds():
        plan = _Plan()
        plan.desc = describe(module, type(module).__name__ + ".")
        plan.net, plan.sizes, plan.choice = plan.desc.pack(*choice), {}, choice
        plan.links = _links(module, plan.desc.params)
        _PLANS[module] = plan
    return plan


def _as_tensor(x, tpdv):
    return (torch.from_numpy(x) if isinstance(x, np.ndarray) else x).to(**tpdv)   # the reference's check(x).to(**self.tpdv)


def _tpdv(module):
    tpdv = getattr(module, "tpdv", None)
    return tpdv if tpdv is not None else dict(dtype=torch.float32, device=next(module.parameters()).device)


def _run(module, plan, function, obs, rnn_states, masks, *action):
    N = rnn_states.size(0)
    T = 1 if obs.size(0) == N else obs.size(0) // max(N, 1)   # the GRU layer's rule: as many rows as states means one step
    if N < 1 or T * N != obs.size(0):
        raise ValueError(f"{type(module).__name__}: obs has {obs.size(0)} rows, not a multiple of rnn_states' {N}")
    if obs.dim() != 2 or obs.shape[1] != plan.desc.obs_dim:
        raise ValueError(f"{type(module).__name__}: obs of shape {tuple(obs.shape)}, expected [{T * N}, {plan.desc.obs_dim}]")
    if obs.device.type != "cuda":
        raise UnsupportedPolicy(f"{type(module).__name__}: inputs on {obs.device} (only a CUDA device)")
    params = plan.desc.params
    save = torch.is_grad_enabled() and any(p.requires_grad for p in params)
    tensors = (obs.contiguous(), rnn_states.reshape(N, HID).contiguous(), masks.reshape(T * N).contiguous()) + tuple(a.contiguous() for a in action)
    return function.apply(*tensors, *params, NetCall(plan.net, N, T, save, plan.sizes)), T * N


def _device_actor_evaluate_actions(self, obs, rnn_states, action, masks, active_masks=None):
    """PPOActor.evaluate_actions as one device call (use_device_networks)."""
    tpdv = _tpdv(self)
    obs, rnn_states, action, masks = (_as_tensor(t, tpdv) for t in (obs, rnn_states, action, masks))
    if active_masks is not None:
        active_masks = _as_tensor(active_masks, tpdv)
    if obs.requires_grad or rnn_states.requires_grad:   # the one call computes no gradient for them
        return self._device_net_original(obs, rnn_states, action, masks, active_masks)
    plan = _plan(self)
    cols = len(plan.desc.nvec) + plan.desc.n_shoot
    if action.dim() != 2 or tuple(action.shape) != (obs.size(0), cols):
        raise ValueError(f"{type(self).__name__}: action of shape {tuple(action.shape)}, expected {(obs.size(0), cols)}")
    (logp, ent), M = _run(self, plan, DeviceActorEvalFunction, obs, rnn_states, masks, action)
    logp, ent = logp.view(M, 1), ent.view(M, 1)
    if active_masks is not None:
        return logp, ent * active_masks / active_masks.sum()
    return logp, ent / M


def _device_critic_forward(self, obs, rnn_states, masks):
    """PPOCritic.forward as one device call (use_device_networks)."""
    tpdv = _tpdv(self)
    obs, rnn_states, masks = (_as_tensor(t, tpdv) for t in (obs, rnn_states, masks))
    if obs.requires_grad or rnn_states.requires_grad:
        return self._device_net_original(obs, rnn_states, masks)
    (values, h_T), _ = _run(self, _plan(self), DeviceCriticFunction, obs, rnn_states, masks)
    return values, h_T.view(-1, 1, HID)


_METHODS = {"actor": ("evaluate_actions", _device_actor_evaluate_actions), "critic": ("forward", _device_critic_forward)}


def _carried(layer, name, default="fp32"):
    value = getattr(layer, name, default)
    return value if isinstance(value, str) else default


def use_device_networks(policy, products=None, dense_products=None, mlp_products=None):
    """Make ``actor.evaluate_actions`` and ``critic.forward`` of ``policy`` run as one device call each, forward and backward.
    ``policy`` is an object with ``actor`` / ``critic`` modules (the reference's PPO and MAPPO ``PPOPolicy``) or one such module. The
    methods are bound in the instance ``__dict__``; module objects, Parameters, ``state_dict`` keys and the optimiser stay as they are,
    ``copy.deepcopy`` of a patched module runs the device method on the copy's own parameters, and it does not matter whether
    ``use_device_mlp`` / ``use_device_gru_layer`` / ``use_device_act`` were applied before. The bound methods keep the reference's
    signatures, return shapes, numpy handling, T = 1 rule and entropy scaling; a call whose obs or rnn_states requires grad goes to the
    module's original method, which is kept. A Parameter or child module that is replaced later is picked up at the next call; a child
    that is ADDED later (a ``feature_norm``) is seen after another ``use_device_networks``.

    ``products`` (the GRU's recurrence), ``dense_products`` (its dense products) and ``mlp_products`` (the MLP blocks) are "fp32" or
    "bf16x3" (anything else: ValueError before a module is looked at); None keeps what a swapped layer already carries (``rnn.products``,
    ``rnn.dense_products``, ``base.mlp.products``) and otherwise means "fp32".

    Everything is checked before anything is changed; UnsupportedPolicy names the module path of whatever cannot run: what ``check_fc``,
    ``check_layer`` and ``check_heads`` refuse, more than 4 blocks in an MLP, a ``value_out`` other than Linear(128, 1) with bias, a
    ``feature_norm`` over another width than the input's, ``use_recurrent_policy=False``, shoot heads without ``use_prior``. Returns
    the number of networks changed."""
    for value, name in ((products, "products"), (dense_products, "dense_products"), (mlp_products, "mlp_products")):
        if value is not None:
            products_code(value, name)
    todo = []
    for root, prefix in policy_roots(policy):
        desc = describe(root, prefix, device=False)
        rnn, mlp = root.rnn, root.base.mlp
        head = _head_mlp(root.act if desc.kind == "actor" else root)
        choice = {"products": products or _carried(rnn, "products"), "dense_products": dense_products or _carried(rnn, "dense_products"),
                  "mlp_products": mlp_products or _carried(mlp, "products")}
        if mlp_products is None and head is not None and _carried(head, "products") != choice["mlp_products"]:
            where = prefix + ("act.mlp" if desc.kind == "actor" else "mlp")
            raise UnsupportedPolicy(f"{where}: products {_carried(head, 'products')!r} but {prefix}base.mlp has {choice['mlp_products']!r} "
                                    "(one choice per network: pass mlp_products)")
        todo.append((root, desc.kind, choice))
    for root, kind, choice in todo:
        name, method = _METHODS[kind]
        if getattr(root.__dict__.get(name), "__func__", None) is not method:
            root._device_net_original = getattr(root, name)   # (bound methods in __dict__: deepcopy rebinds them to the copy)
            setattr(root, name, types.MethodType(method, root))
        root._device_net = choice
        _PLANS.pop(root, None)   # read again at the next call: a child that was added since (a feature_norm) is seen then
    return len(todo)
