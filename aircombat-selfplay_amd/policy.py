"""The reference's PPO rollout policy on the device (``PPOPolicy.get_actions`` / ``.act``, algorithms/ppo/ppo_policy.py).

``DevicePolicy`` runs the actor and critic of the recurrent MLP policy -- hidden sizes ``"128 128"``, one GRU layer of 128, ReLU --
with its sampling and log-probs in one HIP launch (csrc/policy_kernel.hpp). Supported action spaces: ``MultiDiscrete(nvec)`` with up
to 160 logits, and ``Tuple(MultiDiscrete(nvec), MultiDiscrete([2, 2, 2, 2]))`` (the four ``BetaShootBernoulli`` munition heads, which
need ``use_prior``). Everything else raises ``UnsupportedPolicy`` at creation ("The PPO rollout policy").

Sampling is not torch's: a non-deterministic call draws one uniform per (seed, call counter, row, head) from a keyed counter-based
generator (``draw_host`` recomputes any draw) and picks by inverse CDF. The counter advances by one per call.

Weight blobs (fp32) follow the state_dict tensors in the order ``blob_keys`` lists: actor, then critic.

``DeviceMAPPOPolicy`` is the MAPPO form (algorithms/mappo/ppo_policy.py): the same actor, with input widths up to 640, and a critic on
``cent_obs`` / ``share_obs`` (up to 640 wide), fed either explicit rows or, straight from an env, each env's whole observation block.

``DevicePolicyPool`` holds many actors of either form (the self-play opponents) and acts for every env with its assigned member in one
launch.
"""
import ctypes as C

import numpy as np

from .capi import load_library, AC_CTL_FAST, AC_CTL_FP32, AC_CENT_EXPLICIT, AC_CENT_ENV_SHARE, AC_POOL_PPO, AC_POOL_MAPPO

HID = 128


class UnsupportedPolicy(ValueError):
    """A policy configuration or action space the device kernel does not implement (refused at creation)."""


class AcPolicyConfig(C.Structure):
    _fields_ = [("obs_dim", C.c_int32), ("n_cat", C.c_int32), ("nvec", C.c_int32 * 8), ("n_shoot", C.c_int32), ("single_shoot", C.c_int32),
                ("hidden_size", C.c_int32 * 2), ("act_hidden_size", C.c_int32 * 2), ("recurrent_hidden_size", C.c_int32),
                ("recurrent_hidden_layers", C.c_int32), ("activation_id", C.c_int32), ("use_recurrent_policy", C.c_int32),
                ("use_feature_normalization", C.c_int32), ("use_prior", C.c_int32), ("precision", C.c_int32), ("has_critic", C.c_int32)]


class AcPolicyMappoConfig(C.Structure):
    _fields_ = [("base", AcPolicyConfig), ("cent_obs_dim", C.c_int32)]


class AcPolicyRows(C.Structure):
    _fields_ = [("n", C.c_int64), ("na", C.c_int32), ("A", C.c_int32), ("a0", C.c_int32), ("act_stride", C.c_int32)]


def _sizes(s, what):
    try:
        v = [int(x) for x in str(s).split()]
    except ValueError:
        raise UnsupportedPolicy(f"unsupported {what} {s!r}")
    if len(v) != 2:
        raise UnsupportedPolicy(f"unsupported hidden sizes: {what} {s!r} (only \"128 128\")")
    return v


def _action_heads(act_space):
    """(nvec, n_shoot, single_shoot) of a gymnasium (or the env's stand-in) action space."""
    name = type(act_space).__name__
    if name in ("Box", "_Box"):
        raise UnsupportedPolicy("unsupported action space Box (DiagGaussian heads)")
    if name == "MultiBinary":
        raise UnsupportedPolicy("unsupported action space MultiBinary (Bernoulli heads)")
    if name in ("Discrete", "_Discrete"):
        raise UnsupportedPolicy("unsupported action space Discrete")
    if name in ("MultiDiscrete", "_MultiDiscrete"):
        return [int(x) for x in np.asarray(act_space.nvec).ravel()], 0, 0
    if isinstance(act_space, tuple) or name == "Tuple":
        parts = list(act_space.spaces if hasattr(act_space, "spaces") else act_space)
        if len(parts) == 2 and type(parts[0]).__name__ in ("MultiDiscrete", "_MultiDiscrete"):
            nvec = [int(x) for x in np.asarray(parts[0].nvec).ravel()]
            second = type(parts[1]).__name__
            if second in ("Discrete", "_Discrete"):
                return nvec, 0, 1
            if second in ("MultiDiscrete", "_MultiDiscrete"):
                mv = [int(x) for x in np.asarray(parts[1].nvec).ravel()]
                if mv != [2, 2, 2, 2]:
                    raise UnsupportedPolicy(f"unsupported munition part MultiDiscrete({mv}) (only [2, 2, 2, 2])")
                return nvec, 4, 0
    raise UnsupportedPolicy(f"unsupported action space {act_space!r}")


def make_config(obs_space, act_space, args, precision="fast", has_critic=True):
    """The C configuration from the reference's args fields and spaces (no device needed)."""
    if precision not in ("fast", "fp32"):
        raise ValueError("precision is 'fast' or 'fp32'")
    obs_dim = int(np.prod(obs_space.shape))
    nvec, n_shoot, single = _action_heads(act_space)
    c = AcPolicyConfig()
    c.obs_dim = obs_dim
    c.n_cat = min(len(nvec), 8)
    for i, n in enumerate(nvec[:8]):
        c.nvec[i] = n
    if len(nvec) > 8:
        c.n_cat = 9   # refused by the library
    c.n_shoot, c.single_shoot = n_shoot, single
    c.hidden_size[:] = _sizes(getattr(args, "hidden_size", "128 128"), "hidden_size")
    c.act_hidden_size[:] = _sizes(getattr(args, "act_hidden_size", "128 128"), "act_hidden_size")
    c.recurrent_hidden_size = int(getattr(args, "recurrent_hidden_size", 128))
    c.recurrent_hidden_layers = int(getattr(args, "recurrent_hidden_layers", 1))
    c.activation_id = int(getattr(args, "activation_id", 1))
    c.use_recurrent_policy = int(bool(getattr(args, "use_recurrent_policy", True)))
    c.use_feature_normalization = int(bool(getattr(args, "use_feature_normalization", False)))
    c.use_prior = int(bool(getattr(args, "use_prior", False)))
    c.precision = AC_CTL_FP32 if precision == "fp32" else AC_CTL_FAST
    c.has_critic = int(bool(has_critic))
    return c


def check_config(cfg, lib=None):
    """Raise UnsupportedPolicy if the library refuses ``cfg``; else (actor floats, critic floats) of the source blobs."""
    lib = lib or load_library()
    na, nc = C.c_int64(), C.c_int64()
    if lib.ac_policy_blob_floats(C.byref(cfg), C.byref(na), C.byref(nc)) != 0:
        raise UnsupportedPolicy(lib.last_error())
    return int(na.value), int(nc.value)


def make_mappo_config(obs_space, cent_obs_space, act_space, args, precision="fast", has_critic=True):
    """The MAPPO configuration: make_config's fields plus the critic's input width."""
    c = AcPolicyMappoConfig()
    c.base = make_config(obs_space, act_space, args, precision, has_critic)
    c.cent_obs_dim = int(np.prod(cent_obs_space.shape))
    return c


def check_mappo_config(cfg, lib=None):
    """check_config for an AcPolicyMappoConfig: UnsupportedPolicy naming the field, else the blob lengths."""
    lib = lib or load_library()
    na, nc = C.c_int64(), C.c_int64()
    if lib.ac_policy_mappo_blob_floats(C.byref(cfg), C.byref(na), C.byref(nc)) != 0:
        raise UnsupportedPolicy(lib.last_error())
    return int(na.value), int(nc.value)


def _trunk_keys(cfg, prefix_base="base.", prefix_rnn="rnn."):
    k = []
    if cfg.use_feature_normalization:
        k += [prefix_base + "feature_norm.weight", prefix_base + "feature_norm.bias"]
    for i in (0, 2, 3, 5):
        k += [f"{prefix_base}mlp.fc.{i}.weight", f"{prefix_base}mlp.fc.{i}.bias"]
    k += [prefix_rnn + "gru.weight_ih_l0", prefix_rnn + "gru.weight_hh_l0", prefix_rnn + "gru.bias_ih_l0", prefix_rnn + "gru.bias_hh_l0",
          prefix_rnn + "norm.weight", prefix_rnn + "norm.bias"]
    return k


def blob_keys(cfg):
    """(actor keys, critic keys): the state_dict tensors of each blob, in blob order."""
    actor = _trunk_keys(cfg)
    for i in (0, 2, 3, 5):
        actor += [f"act.mlp.fc.{i}.weight", f"act.mlp.fc.{i}.bias"]
    for h in range(cfg.n_cat):
        actor += [f"act.action_outs.{h}.logits_net.weight", f"act.action_outs.{h}.logits_net.bias"]
    for s in range(cfg.n_shoot):
        actor += [f"act.action_outs.{cfg.n_cat + s}.net.weight", f"act.action_outs.{cfg.n_cat + s}.net.bias"]
    critic = _trunk_keys(cfg)
    for i in (0, 2, 3, 5):
        critic += [f"mlp.fc.{i}.weight", f"mlp.fc.{i}.bias"]
    critic += ["value_out.weight", "value_out.bias"]
    return actor, critic


def _load_sd(sd):
    if isinstance(sd, (str, bytes)) or hasattr(sd, "__fspath__"):
        import torch
        sd = torch.load(sd, map_location="cpu")
    return sd


def blob_from_state_dict(cfg, sd, critic=False):
    """fp32 numpy blob of one network from its state_dict (torch tensors or arrays)."""
    keys = blob_keys(cfg)[1 if critic else 0]
    missing = [k for k in keys if k not in sd]
    if missing:
        raise KeyError(f"state_dict lacks {missing[:4]}{' ...' if len(missing) > 4 else ''}")
    parts = []
    for k in keys:
        v = sd[k]
        v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        parts.append(np.asarray(v, dtype=np.float32).ravel())
    return np.concatenate(parts)


def draw_host(seed, counter, rows, head, lib=None):
    """The uniforms of rows ``rows`` (a range or an int count) for one head, as the kernel draws them."""
    lib = lib or load_library()
    if isinstance(rows, int):
        rows = range(rows)
    r0, n = rows.start, len(rows)
    out = np.empty(n, dtype=np.float32)
    lib.check(lib.ac_policy_draw_host(C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint64(int(counter) & (2 ** 64 - 1)), int(r0), n,
                                      int(head), out.ctypes.data), "ac_policy_draw_host")
    return out


class DevicePolicy:
    """PPOPolicy.get_actions / act on the device (module docstring).

    ``args`` carries the reference's fields ``hidden_size``, ``act_hidden_size``, ``recurrent_hidden_size``, ``recurrent_hidden_layers``,
    ``activation_id``, ``use_feature_normalization``, ``use_prior`` (and ``use_recurrent_policy``). ``precision``: ``"fast"`` (two fp16
    pieces per product, AC_CTL_FAST) or ``"fp32"`` (three bf16 pieces, AC_CTL_FP32). ``critic=False`` builds an actor-only policy (a
    self-play opponent)."""

    def __init__(self, obs_space, act_space, args, device_id=0, precision="fast", seed=0, critic=True):
        self.lib = load_library()
        self.cfg = make_config(obs_space, act_space, args, precision, critic)
        self.actor_floats, self.critic_floats = check_config(self.cfg, self.lib)
        self.obs_dim = int(self.cfg.obs_dim)
        self.n_heads = int(self.cfg.n_cat + self.cfg.n_shoot)
        self.has_critic = bool(critic)
        self.device_id = int(device_id)
        self.precision = precision
        self.seed = int(seed)
        self.counter = 0
        h = C.c_void_p()
        self.lib.check(self.lib.ac_policy_create(self.device_id, C.byref(self.cfg), C.byref(h)), "ac_policy_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.lib.ac_policy_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights
    def load_state_dict(self, actor_sd, critic_sd=None):
        """The reference's state_dicts (or paths of .pt files), host path."""
        a = blob_from_state_dict(self.cfg, _load_sd(actor_sd))
        c = blob_from_state_dict(self.cfg, _load_sd(critic_sd), critic=True) if critic_sd is not None else None
        self.load_blobs(a, c)

    def load_blobs(self, actor, critic=None):
        a = np.ascontiguousarray(actor, dtype=np.float32)
        c = None if critic is None else np.ascontiguousarray(critic, dtype=np.float32)
        self.lib.check(self.lib.ac_policy_load(self._h, a.ctypes.data, a.size, None if c is None else c.ctypes.data,
                                               0 if c is None else c.size), "ac_policy_load")

    def load_from_torch(self, actor_module, critic_module=None, check=True):
        """Weights from torch modules (or state_dicts) already on this GPU: concatenated on torch's stream and packed on the device,
        with no host round trip. A refused load (a non-finite weight; |w| >= 65504 in the fast form) leaves the previous weights in
        place; with ``check`` it raises (one 8-byte read after the stream)."""
        import torch

        def dev_blob(m, critic):
            sd = m.state_dict() if hasattr(m, "state_dict") else m
            keys = blob_keys(self.cfg)[1 if critic else 0]
            return torch.cat([sd[k].detach().reshape(-1).to(torch.float32) for k in keys]).contiguous()

        a = dev_blob(actor_module, False)
        c = dev_blob(critic_module, True) if critic_module is not None else None
        stream = torch.cuda.current_stream(a.device).cuda_stream
        self.lib.check(self.lib.ac_policy_load_device(self._h, stream, a.data_ptr(), a.numel(), None if c is None else c.data_ptr(),
                                                      0 if c is None else c.numel()), "ac_policy_load_device")
        self._keep = (a, c)   # alive until the packing kernel has run (torch's caching allocator reuses freed blocks in stream order)
        if check:
            ra, rc = C.c_int32(), C.c_int32()
            self.lib.check(self.lib.ac_policy_load_refused(self._h, stream, C.byref(ra), C.byref(rc)), "ac_policy_load_refused")
            if ra.value or (c is not None and rc.value):
                raise ValueError("load_from_torch: weights refused (non-finite, or |w| >= 65504 in the fast form); previous weights kept")

    def packed(self, net=0):
        """The packed weights of the actor (0) / critic (1) as a torch uint8 tensor copy (test aid)."""
        import torch
        p, n = C.c_void_p(), C.c_int64()
        self.lib.check(self.lib.ac_policy_packed(self._h, int(net), C.byref(p), C.byref(n)), "ac_policy_packed")
        holder = type("_Packed", (), {})()
        holder.__cuda_array_interface__ = {"shape": (int(n.value) * 4,), "typestr": "|u1", "data": (p.value, False), "version": 2}
        return torch.as_tensor(holder, device=f"cuda:{self.device_id}").clone()

    # ---- calls
    def _launch(self, rows, obs, h_a, h_c, masks, deterministic, values, actions, logp, h_a_out, h_c_out, counter):
        import torch
        ptr = lambda t: None if t is None else t.data_ptr()
        stream = torch.cuda.current_stream(torch.device("cuda", self.device_id)).cuda_stream
        if counter is None:
            counter = self.counter
            self.counter += 1
        self.lib.check(self.lib.ac_policy_get_actions(
            self._h, stream, C.byref(rows), ptr(obs), ptr(h_a), ptr(h_c), ptr(masks), int(bool(deterministic)),
            C.c_uint64(self.seed & (2 ** 64 - 1)), C.c_uint64(int(counter) & (2 ** 64 - 1)), ptr(values), ptr(actions), ptr(logp),
            ptr(h_a_out), ptr(h_c_out)), "ac_policy_get_actions")
        return counter

    def _tensor(self, x, shape_tail):
        import torch
        dev = torch.device("cuda", self.device_id)
        was_np = not isinstance(x, torch.Tensor)
        t = torch.as_tensor(np.asarray(x, dtype=np.float32) if was_np else x).to(device=dev, dtype=torch.float32)
        t = t.reshape((-1,) + shape_tail).contiguous()
        return t, was_np

    def get_actions(self, obs, rnn_states_actor, rnn_states_critic, masks, deterministic=False, counter=None):
        """values [N, 1], actions [N, n_heads] (float32), action_log_probs [N, 1], rnn_states_actor / _critic [N, 1, 128] -- like
        PPOPolicy.get_actions. torch tensors in give torch tensors out (ordered on torch's current stream); numpy in, numpy out."""
        import torch
        if not self.has_critic:
            raise RuntimeError("get_actions: the policy was created without a critic (use act)")
        o, was_np = self._tensor(obs, (self.obs_dim,))
        n = o.shape[0]
        ha, _ = self._tensor(rnn_states_actor, (HID,))
        hc, _ = self._tensor(rnn_states_critic, (HID,))
        m, _ = self._tensor(masks, ())
        if ha.shape[0] != n or hc.shape[0] != n or m.shape[0] != n:
            raise ValueError("get_actions: obs, rnn states and masks disagree on the number of rows")
        dev = o.device
        values = torch.empty((n, 1), device=dev)
        actions = torch.empty((n, self.n_heads), device=dev)
        logp = torch.empty((n, 1), device=dev)
        ha_out = torch.empty((n, 1, HID), device=dev)
        hc_out = torch.empty((n, 1, HID), device=dev)
        self.last_counter = self._launch(AcPolicyRows(n, 0, 0, 0, self.n_heads), o, ha, hc, m, deterministic, values, actions, logp,
                                         ha_out, hc_out, counter)
        out = (values, actions, logp, ha_out, hc_out)
        if was_np:
            torch.cuda.current_stream(dev).synchronize()
            return tuple(t.cpu().numpy() for t in out)
        return out

    def get_values(self, obs, rnn_states_critic, masks):
        """values [N, 1] -- PPOPolicy.get_values: the critic alone (one launch of critic workgroups), bit-identical to get_actions' values."""
        o, was_np = self._tensor(obs, (self.obs_dim,))
        return self._values(AcPolicyRows(o.shape[0], 0, 0, 0, self.n_heads), o, AC_CENT_EXPLICIT, rnn_states_critic, masks, was_np)

    def _values(self, rows, inp, mode, rnn_states_critic, masks, was_np, rnn_states_out=None):
        import torch
        if not self.has_critic:
            raise RuntimeError("get_values: the policy was created without a critic")
        n = int(rows.n)
        hc, _ = self._tensor(rnn_states_critic, (HID,))
        m, _ = self._tensor(masks, ())
        if hc.shape[0] != n or m.shape[0] != n:
            raise ValueError("get_values: inputs, rnn states and masks disagree on the number of rows")
        values = torch.empty((n, 1), device=hc.device)
        hc_out = torch.empty((n, 1, HID), device=hc.device) if rnn_states_out is None else rnn_states_out
        stream = torch.cuda.current_stream(hc.device).cuda_stream
        self.lib.check(self.lib.ac_policy_get_values(self._h, stream, C.byref(rows), inp.data_ptr(), int(mode), hc.data_ptr(), m.data_ptr(),
                                                     values.data_ptr(), hc_out.data_ptr()), "ac_policy_get_values")
        self._keep_values = (inp, hc, m)   # (the inputs stay alive until the launch has run: torch frees in stream order)
        if was_np:
            torch.cuda.current_stream(hc.device).synchronize()
            return values.cpu().numpy()
        return values

    def act(self, obs, rnn_states_actor, masks, deterministic=False, counter=None, return_log_probs=False):
        """actions [N, n_heads], rnn_states_actor [N, 1, 128] -- PPOPolicy.act (actor only); with ``return_log_probs`` also the log-probs."""
        import torch
        o, was_np = self._tensor(obs, (self.obs_dim,))
        n = o.shape[0]
        ha, _ = self._tensor(rnn_states_actor, (HID,))
        m, _ = self._tensor(masks, ())
        if ha.shape[0] != n or m.shape[0] != n:
            raise ValueError("act: obs, rnn states and masks disagree on the number of rows")
        dev = o.device
        actions = torch.empty((n, self.n_heads), device=dev)
        logp = torch.empty((n, 1), device=dev)
        ha_out = torch.empty((n, 1, HID), device=dev)
        self.last_counter = self._launch(AcPolicyRows(n, 0, 0, 0, self.n_heads), o, ha, None, m, deterministic, None, actions, logp,
                                         ha_out, None, counter)
        out = (actions, ha_out, logp) if return_log_probs else (actions, ha_out)
        if was_np:
            torch.cuda.current_stream(dev).synchronize()
            return tuple(t.cpu().numpy() for t in out)
        return out

    def act_into_env(self, env, rnn_states, masks, agents=None, deterministic=False, counter=None, rnn_states_out=None):
        """Actions of agents ``agents`` (a slice [a0, a1) of every env) written straight into ``env``'s device action buffer (ready for
        ``env.step_device(stream=torch.cuda.current_stream())``), reading their observations from the env's device obs buffer.
        ``rnn_states`` / ``masks``: torch tensors on the GPU, [E * (a1 - a0), 1, 128] / [E * (a1 - a0), 1], in (env, agent) order; the
        new states go to ``rnn_states_out`` (default: in place). Returns (rnn_states_out, log-probs [E * (a1 - a0), 1])."""
        import torch
        E, A = env.num_envs, env.num_agents
        a0, a1, step = (agents or slice(0, A)).indices(A)
        if step != 1 or a1 <= a0:
            raise ValueError("act_into_env: agents must be a contiguous, non-empty slice")
        if env.obs_dim != self.obs_dim or env.act_dim < self.n_heads:
            raise ValueError(f"act_into_env: env obs_dim {env.obs_dim} / act_dim {env.act_dim} do not fit this policy")
        act, obs, _, _, _ = env.device_tensors()
        n = E * (a1 - a0)
        if rnn_states.numel() != n * HID or masks.numel() != n or not rnn_states.is_contiguous() or not masks.is_contiguous():
            raise ValueError("act_into_env: rnn_states / masks must be contiguous [E * (a1 - a0), 1, 128] / [E * (a1 - a0), 1]")
        out = rnn_states if rnn_states_out is None else rnn_states_out
        logp = torch.empty((n, 1), device=obs.device)
        self.last_counter = self._launch(AcPolicyRows(n, a1 - a0, A, a0, env.act_dim), obs, rnn_states, None, masks, deterministic, None,
                                         act, logp, out, None, counter)
        return out, logp


class DeviceMAPPOPolicy(DevicePolicy):
    """The MAPPO PPOPolicy (algorithms/mappo/ppo_policy.py) on the device: DevicePolicy's actor for observations up to 640 wide, and a
    critic on ``cent_obs`` (``share_obs``, up to 640 wide). ``get_actions`` / ``get_values`` take explicit ``cent_obs`` rows;
    ``get_actions_into_env`` / ``get_values_from_env`` let the critic read each env's observation block in the env's device buffer
    (``cent_obs_space`` must then be ``num_agents * obs_dim`` wide), so ``share_obs`` is never built. ``act`` / ``act_into_env``, the
    weight loads and ``packed`` are DevicePolicy's. Blobs: ``blob_keys``; the critic's ``base.mlp.fc.0.weight`` is [128, cent_obs_dim]."""

    def __init__(self, obs_space, cent_obs_space, act_space, args, device_id=0, precision="fast", seed=0, critic=True):
        self.lib = load_library()
        self.mcfg = make_mappo_config(obs_space, cent_obs_space, act_space, args, precision, critic)
        self.cfg = self.mcfg.base
        self.actor_floats, self.critic_floats = check_mappo_config(self.mcfg, self.lib)
        self.obs_dim = int(self.cfg.obs_dim)
        self.cent_obs_dim = int(self.mcfg.cent_obs_dim)
        self.n_heads = int(self.cfg.n_cat + self.cfg.n_shoot)
        self.has_critic = bool(critic)
        self.device_id = int(device_id)
        self.precision = precision
        self.seed = int(seed)
        self.counter = 0
        h = C.c_void_p()
        self.lib.check(self.lib.ac_policy_mappo_create(self.device_id, C.byref(self.mcfg), C.byref(h)), "ac_policy_mappo_create")
        self._h = h

    def _launch(self, rows, obs, h_a, h_c, masks, deterministic, values, actions, logp, h_a_out, h_c_out, counter, cin=None,
                mode=AC_CENT_EXPLICIT):
        import torch
        ptr = lambda t: None if t is None else t.data_ptr()
        stream = torch.cuda.current_stream(torch.device("cuda", self.device_id)).cuda_stream
        if counter is None:
            counter = self.counter
            self.counter += 1
        self.lib.check(self.lib.ac_policy_get_actions_mappo(
            self._h, stream, C.byref(rows), ptr(obs), ptr(cin), int(mode), ptr(h_a), ptr(h_c), ptr(masks), int(bool(deterministic)),
            C.c_uint64(self.seed & (2 ** 64 - 1)), C.c_uint64(int(counter) & (2 ** 64 - 1)), ptr(values), ptr(actions), ptr(logp),
            ptr(h_a_out), ptr(h_c_out)), "ac_policy_get_actions_mappo")
        return counter

    def get_actions(self, cent_obs, obs, rnn_states_actor, rnn_states_critic, masks, deterministic=False, counter=None):
        """values [N, 1], actions [N, n_heads] (float32), action_log_probs [N, 1], rnn_states_actor / _critic [N, 1, 128] -- like the
        MAPPO PPOPolicy.get_actions. torch in, torch out (on torch's current stream); numpy in, numpy out."""
        import torch
        if not self.has_critic:
            raise RuntimeError("get_actions: the policy was created without a critic (use act)")
        o, was_np = self._tensor(obs, (self.obs_dim,))
        n = o.shape[0]
        co, _ = self._tensor(cent_obs, (self.cent_obs_dim,))
        ha, _ = self._tensor(rnn_states_actor, (HID,))
        hc, _ = self._tensor(rnn_states_critic, (HID,))
        m, _ = self._tensor(masks, ())
        if co.shape[0] != n or ha.shape[0] != n or hc.shape[0] != n or m.shape[0] != n:
            raise ValueError("get_actions: cent_obs, obs, rnn states and masks disagree on the number of rows")
        dev = o.device
        values = torch.empty((n, 1), device=dev)
        actions = torch.empty((n, self.n_heads), device=dev)
        logp = torch.empty((n, 1), device=dev)
        ha_out = torch.empty((n, 1, HID), device=dev)
        hc_out = torch.empty((n, 1, HID), device=dev)
        self.last_counter = self._launch(AcPolicyRows(n, 0, 0, 0, self.n_heads), o, ha, hc, m, deterministic, values, actions, logp,
                                         ha_out, hc_out, counter, cin=co)
        self._keep_call = (o, co, ha, hc, m)
        out = (values, actions, logp, ha_out, hc_out)
        if was_np:
            torch.cuda.current_stream(dev).synchronize()
            return tuple(t.cpu().numpy() for t in out)
        return out

    def get_values(self, cent_obs, rnn_states_critic, masks):
        """values [N, 1] -- the MAPPO PPOPolicy.get_values (critic workgroups only; bit-identical to get_actions' values)."""
        co, was_np = self._tensor(cent_obs, (self.cent_obs_dim,))
        return self._values(AcPolicyRows(co.shape[0], 0, 0, 0, self.n_heads), co, AC_CENT_EXPLICIT, rnn_states_critic, masks, was_np)

    def _env_rows(self, env, agents, what):
        E, A = env.num_envs, env.num_agents
        a0, a1, step = (agents or slice(0, A)).indices(A)
        if step != 1 or a1 <= a0:
            raise ValueError(f"{what}: agents must be a contiguous, non-empty slice")
        if env.obs_dim != self.obs_dim or env.act_dim < self.n_heads:
            raise ValueError(f"{what}: env obs_dim {env.obs_dim} / act_dim {env.act_dim} do not fit this policy")
        if self.has_critic and self.cent_obs_dim != A * self.obs_dim:
            raise UnsupportedPolicy(f"{what}: cent_obs_space is {self.cent_obs_dim} wide, the env share input is num_agents * obs_dim = "
                                    f"{A} * {self.obs_dim} = {A * self.obs_dim}")
        return E * (a1 - a0), AcPolicyRows(E * (a1 - a0), a1 - a0, A, a0, env.act_dim)

    @staticmethod
    def _check_rows(n, what, **ts):
        for name, t in ts.items():
            if t.numel() != n * (HID if name.startswith("rnn") else 1) or not t.is_contiguous():
                raise ValueError(f"{what}: {name} must be contiguous with {n} rows (E * (a1 - a0), in (env, agent) order)")

    def get_actions_into_env(self, env, rnn_states_actor, rnn_states_critic, masks, agents=None, deterministic=False, counter=None,
                             rnn_states_actor_out=None, rnn_states_critic_out=None):
        """get_actions for agents ``agents`` (a slice [a0, a1) of every env) of a HipShareVecEnv on the device: the actor reads their rows
        of the env's obs buffer, the critic each env's whole observation block (share_obs, never built), and the actions go straight
        into the env's device action buffer. States / masks: contiguous torch tensors [E * (a1 - a0), 1, 128] / [E * (a1 - a0), 1];
        the new states go to the ``*_out`` tensors (default: in place). Returns (values, log-probs, rnn_states_actor, rnn_states_critic)."""
        import torch
        if not self.has_critic:
            raise RuntimeError("get_actions_into_env: the policy was created without a critic (use act_into_env)")
        n, rows = self._env_rows(env, agents, "get_actions_into_env")
        self._check_rows(n, "get_actions_into_env", rnn_states_actor=rnn_states_actor, rnn_states_critic=rnn_states_critic, masks=masks)
        act, obs, _, _, _ = env.device_tensors()
        ha_out = rnn_states_actor if rnn_states_actor_out is None else rnn_states_actor_out
        hc_out = rnn_states_critic if rnn_states_critic_out is None else rnn_states_critic_out
        values = torch.empty((n, 1), device=obs.device)
        logp = torch.empty((n, 1), device=obs.device)
        self.last_counter = self._launch(rows, obs, rnn_states_actor, rnn_states_critic, masks, deterministic, values, act, logp, ha_out,
                                         hc_out, counter, mode=AC_CENT_ENV_SHARE)
        return values, logp, ha_out, hc_out

    def get_values_from_env(self, env, rnn_states_critic, masks, agents=None):
        """values [E * (a1 - a0), 1] of agents ``agents`` with each env's observation block as the critic input (the runner's compute()
        on the last observations)."""
        n, rows = self._env_rows(env, agents, "get_values_from_env")
        self._check_rows(n, "get_values_from_env", rnn_states_critic=rnn_states_critic, masks=masks)
        _, obs, _, _, _ = env.device_tensors()
        return self._values(rows, obs, AC_CENT_ENV_SHARE, rnn_states_critic, masks, False)


class DevicePolicyPool:
    """A pool of ``capacity`` actors on the device, the self-play opponents of the reference's runners, acted for in one launch
    (csrc/policy_pool.hpp). Every member is packed as ``DevicePolicy`` (``form="ppo"``) or ``DeviceMAPPOPolicy`` (``form="mappo"``)
    packs its actor, with one precision for the whole pool. ``assign`` maps each env to a member (-1: not acted for); ``act_into_env`` /
    ``act`` then act for every assigned row with its member's weights, with ``DevicePolicy``'s sampling: draws keyed by (seed, counter,
    row of the call, head), so each row's output is the one a DevicePolicy holding that member would give in the same call.
    ``assign_sides`` maps each *side* of each env to a member instead, for the one whole-range launch of a league (league.py).

    The host-side choice of opponents (``selfplay_algo.choose``, the ELO update) stays the reference's: the runner maps its policy-pool
    keys to member indices, loads them, and calls ``assign``. Assign after loading: a member's load state is
    read when the assignment is planned."""

    def __init__(self, obs_space, act_space, args, capacity, form="ppo", precision="fast", seed=0, device_id=0):
        if form not in ("ppo", "mappo"):
            raise ValueError("form is 'ppo' or 'mappo'")
        self.lib = load_library()
        self.cfg = make_config(obs_space, act_space, args, precision, has_critic=False)
        self.form, self._form = form, (AC_POOL_MAPPO if form == "mappo" else AC_POOL_PPO)
        self.capacity = int(capacity)
        ns, npk = C.c_int64(), C.c_int64()
        if self.lib.ac_policy_pool_member_floats(C.byref(self.cfg), self._form, self.capacity, C.byref(ns), C.byref(npk)) != 0:
            raise UnsupportedPolicy(self.lib.last_error())
        self.actor_floats, self.packed_floats = int(ns.value), int(npk.value)
        self.obs_dim = int(self.cfg.obs_dim)
        self.n_heads = int(self.cfg.n_cat + self.cfg.n_shoot)
        self.device_id = int(device_id)
        self.precision = precision
        self.seed = int(seed)
        self.counter = 0
        self._na = 1        # rows per env of the plan (the agent count of the calls)
        self._members = None
        self._sided = None   # (E, A) while a sided plan (assign_sides) is in force
        h = C.c_void_p()
        self.lib.check(self.lib.ac_policy_pool_create(self.device_id, C.byref(self.cfg), self._form, self.capacity, C.byref(h)),
                       "ac_policy_pool_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.lib.ac_policy_pool_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        import torch
        return torch.cuda.current_stream(torch.device("cuda", self.device_id)).cuda_stream

    def _member(self, member):
        m = int(member)
        if not 0 <= m < self.capacity:
            raise ValueError(f"member {m} out of range (capacity {self.capacity})")
        return m

    # ---- members
    def load_state_dict(self, member, actor_sd):
        """Member ``member`` from the reference's actor state_dict (or the path of an ``actor_{episode}.pt``), host path."""
        self.load_blob(member, blob_from_state_dict(self.cfg, _load_sd(actor_sd)))

    def load_blob(self, member, actor):
        a = np.ascontiguousarray(actor, dtype=np.float32)
        self.lib.check(self.lib.ac_policy_pool_load(self._h, self._member(member), a.ctypes.data, a.size), "ac_policy_pool_load")

    def load_from_torch(self, member, actor_module, check=True):
        """Member ``member`` from a torch actor module (or state_dict) on this GPU, packed on the device on torch's stream. A refused load
        (a non-finite weight; |w| >= 65504 in the fast form) keeps the member's previous weights; with ``check`` it raises."""
        import torch
        sd = actor_module.state_dict() if hasattr(actor_module, "state_dict") else actor_module
        a = torch.cat([sd[k].detach().reshape(-1).to(torch.float32) for k in blob_keys(self.cfg)[0]]).contiguous()
        stream = torch.cuda.current_stream(a.device).cuda_stream
        self.lib.check(self.lib.ac_policy_pool_load_device(self._h, stream, self._member(member), a.data_ptr(), a.numel()),
                       "ac_policy_pool_load_device")
        self._keep = a   # alive until the packing kernel has run
        if check:
            r = C.c_int32()
            self.lib.check(self.lib.ac_policy_pool_load_refused(self._h, stream, C.byref(r)), "ac_policy_pool_load_refused")
            if r.value:
                raise ValueError("load_from_torch: weights refused (non-finite, or |w| >= 65504 in the fast form); previous weights kept")

    def copy_from(self, member, device_policy):
        """Member ``member`` := ``device_policy``'s packed actor (a DevicePolicy for the ppo form, a DeviceMAPPOPolicy for the mappo form,
        same configuration and precision), device to device on torch's stream: the learner's actor joins the pool with no file."""
        self.lib.check(self.lib.ac_policy_pool_copy_from(self._h, self._stream(), self._member(member), device_policy._h),
                       "ac_policy_pool_copy_from")

    def packed(self, member):
        """Member ``member``'s packed weights as a torch uint8 tensor copy (test aid)."""
        import torch
        p, n = C.c_void_p(), C.c_int64()
        self.lib.check(self.lib.ac_policy_pool_packed(self._h, self._member(member), C.byref(p), C.byref(n)), "ac_policy_pool_packed")
        holder = type("_Packed", (), {})()
        holder.__cuda_array_interface__ = {"shape": (int(n.value) * 4,), "typestr": "|u1", "data": (p.value, False), "version": 2}
        return torch.as_tensor(holder, device=f"cuda:{self.device_id}").clone()

    def set_tile_order(self, xcd):
        """Deal each member's tiles to workgroups that share one XCD (True, the default) or in member-major order (False); speed only."""
        self.lib.check(self.lib.ac_policy_pool_set_tile_order(self._h, int(bool(xcd))), "ac_policy_pool_set_tile_order")

    # ---- assignment
    def assign(self, members, check=True, na=None):
        """Env e's rows act with member ``members[e]`` (-1: not acted for, their outputs untouched); ``members``: numpy or a torch int
        tensor of length E. Planned on the device on torch's stream and kept for every later call (``na``: rows per env of those calls,
        default the last call's). With ``check``, one sync reads back the plan: a ValueError names the first env whose member is out of
        range or not loaded, and the exact tile count becomes the act launch's grid."""
        import torch
        dev = torch.device("cuda", self.device_id)
        if isinstance(members, torch.Tensor):
            m = members.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        else:
            m = torch.as_tensor(np.ascontiguousarray(np.asarray(members).reshape(-1), dtype=np.int32)).to(dev)
        if na is not None:
            self._na = int(na)
        stream = torch.cuda.current_stream(dev).cuda_stream
        self.lib.check(self.lib.ac_policy_pool_assign(self._h, stream, m.data_ptr(), m.numel(), self._na), "ac_policy_pool_assign")
        self._members = m   # alive until the copy has run
        self._sided = None
        self.num_envs = int(m.numel())
        if check:
            bad, nt = C.c_int32(), C.c_int32()
            self.lib.check(self.lib.ac_policy_pool_check(self._h, stream, C.byref(bad), C.byref(nt)), "ac_policy_pool_check")
            self.num_tiles = int(nt.value)
            if bad.value >= 0:
                v = int(m[bad.value].item())
                why = f"out of range (capacity {self.capacity})" if not 0 <= v < self.capacity else "not loaded"
                raise ValueError(f"assign: env {bad.value} has member {v}, {why}")
        return self

    def assign_sides(self, members2, A, check=True):
        """The sided assignment of a league (league.py): env e's agents ``[0, A/2)`` act with member ``members2[e][0]``, agents
        ``[A/2, A)`` with ``members2[e][1]`` (-1: that side is not acted for); ``members2``: numpy or a torch int tensor of shape
        [E, 2], ``A`` even. Planned on torch's stream like ``assign``. While it is in force only the whole-range call is taken,
        ``act_into_env(env, h, masks, agents=slice(0, A))`` with [E * A, 1, 128] states: one launch for both sides of every env, each
        row with its side's member and its own keyed draws. Other ``agents`` and ``act`` raise ``ValueError``; ``assign`` returns the
        pool to the per-env form. With ``check``, a ValueError names the first env with a member out of range or not loaded."""
        import torch
        dev = torch.device("cuda", self.device_id)
        A = int(A)
        if A < 2 or A % 2:
            raise ValueError(f"assign_sides: A must be even and >= 2 (got {A})")
        if isinstance(members2, torch.Tensor):
            if members2.dim() != 2 or members2.shape[1] != 2 or members2.is_floating_point():
                raise ValueError("assign_sides: members2 must be an int tensor of shape [E, 2]")
            m = members2.to(device=dev, dtype=torch.int32).contiguous()
        else:
            m = np.asarray(members2)
            if m.ndim != 2 or m.shape[1] != 2 or not np.issubdtype(m.dtype, np.integer):
                raise ValueError("assign_sides: members2 must be an int array of shape [E, 2]")
            m = torch.as_tensor(np.ascontiguousarray(m, dtype=np.int32)).to(dev)
        E = int(m.shape[0])
        stream = torch.cuda.current_stream(dev).cuda_stream
        self.lib.check(self.lib.ac_policy_pool_assign_sides(self._h, stream, m.data_ptr(), E, A), "ac_policy_pool_assign_sides")
        self._members = m   # alive until the copy has run
        self._sided, self._na = (E, A), A
        self.num_envs = E
        if check:
            bad, nt = C.c_int32(), C.c_int32()
            self.lib.check(self.lib.ac_policy_pool_check(self._h, stream, C.byref(bad), C.byref(nt)), "ac_policy_pool_check")
            self.num_tiles = int(nt.value)
            if bad.value >= 0:
                pair = [int(v) for v in m[bad.value].tolist()]
                raise ValueError(f"assign_sides: env {bad.value} has members {pair}: out of range (capacity {self.capacity}) or not loaded")
        return self

    def assign_split(self, E, member_ids, check=True, na=None):
        """The reference's split: ``np.array_split(np.arange(E), K)``, range k to ``member_ids[k]``."""
        members = np.empty(int(E), dtype=np.int32)
        for k, idx in enumerate(np.array_split(np.arange(int(E)), len(member_ids))):
            members[idx] = int(member_ids[k])
        return self.assign(members, check=check, na=na)

    # ---- calls
    def _launch(self, rows, obs, h, masks, deterministic, actions, logp, h_out, counter):
        if self._sided is not None and (rows.na, rows.A, rows.a0, rows.n) != (self._sided[1], self._sided[1], 0, self._sided[0] * self._sided[1]):
            raise ValueError(f"a sided plan (assign_sides) for {self._sided[0]} envs of {self._sided[1]} agents is in force: only "
                             "act_into_env(..., agents=slice(0, A)) over every agent of every env is taken (assign() returns to the per-env form)")
        if counter is None:
            counter = self.counter
            self.counter += 1
        self._na = int(rows.na) if rows.na > 0 else 1
        self.lib.check(self.lib.ac_policy_pool_act(
            self._h, self._stream(), C.byref(rows), obs.data_ptr(), h.data_ptr(), masks.data_ptr(), int(bool(deterministic)),
            C.c_uint64(self.seed & (2 ** 64 - 1)), C.c_uint64(int(counter) & (2 ** 64 - 1)), actions.data_ptr(), logp.data_ptr(),
            h_out.data_ptr()), "ac_policy_pool_act")
        return counter

    def act_into_env(self, env, rnn_states, masks, agents=None, deterministic=False, counter=None, rnn_states_out=None, logp_out=None):
        """DevicePolicy.act_into_env for the pool: agents ``agents`` (default the second half, ``slice(A // 2, A)``, the opponents) of
        every env, each env with its assigned member; the actions go straight into ``env``'s device action buffer. ``rnn_states`` /
        ``masks``: contiguous [E * (a1 - a0), 1, 128] / [E * (a1 - a0), 1] torch tensors in (env, agent) order; the new states go to
        ``rnn_states_out`` (default: in place). Returns (rnn_states_out, log-probs [E * (a1 - a0), 1]); the rows of unassigned envs are
        not written in any of them (``logp_out`` may supply the log-prob tensor)."""
        import torch
        E, A = env.num_envs, env.num_agents
        a0, a1, step = (agents or slice(A // 2, A)).indices(A)
        if step != 1 or a1 <= a0:
            raise ValueError("act_into_env: agents must be a contiguous, non-empty slice")
        if env.obs_dim != self.obs_dim or env.act_dim < self.n_heads:
            raise ValueError(f"act_into_env: env obs_dim {env.obs_dim} / act_dim {env.act_dim} do not fit this pool")
        act, obs, _, _, _ = env.device_tensors()
        n = E * (a1 - a0)
        if rnn_states.numel() != n * HID or masks.numel() != n or not rnn_states.is_contiguous() or not masks.is_contiguous():
            raise ValueError("act_into_env: rnn_states / masks must be contiguous [E * (a1 - a0), 1, 128] / [E * (a1 - a0), 1]")
        out = rnn_states if rnn_states_out is None else rnn_states_out
        logp = torch.empty((n, 1), device=obs.device) if logp_out is None else logp_out
        self.last_counter = self._launch(AcPolicyRows(n, a1 - a0, A, a0, env.act_dim), obs, rnn_states, masks, deterministic, act, logp,
                                         out, counter)
        return out, logp

    def act(self, obs, rnn_states, masks, deterministic=False, counter=None, return_log_probs=False):
        """actions [N, n_heads], rnn_states [N, 1, 128] (with ``return_log_probs`` also the log-probs) for explicit rows, row e acting
        with member ``members[e]`` of the assignment (one row per env). Unassigned rows come back zero. torch in, torch out (on torch's
        current stream); numpy in, numpy out."""
        import torch
        dev = torch.device("cuda", self.device_id)
        was_np = not isinstance(obs, torch.Tensor)
        cv = lambda x, tail: torch.as_tensor(np.asarray(x, dtype=np.float32) if not isinstance(x, torch.Tensor) else x).to(
            device=dev, dtype=torch.float32).reshape((-1,) + tail).contiguous()
        o, h, m = cv(obs, (self.obs_dim,)), cv(rnn_states, (HID,)), cv(masks, ())
        n = o.shape[0]
        if h.shape[0] != n or m.shape[0] != n:
            raise ValueError("act: obs, rnn states and masks disagree on the number of rows")
        actions = torch.zeros((n, self.n_heads), device=dev)
        logp = torch.zeros((n, 1), device=dev)
        h_out = torch.zeros((n, 1, HID), device=dev)
        self.last_counter = self._launch(AcPolicyRows(n, 0, 0, 0, self.n_heads), o, h, m, deterministic, actions, logp, h_out, counter)
        self._keep_call = (o, h, m)
        out = (actions, h_out, logp) if return_log_probs else (actions, h_out)
        if was_np:
            torch.cuda.current_stream(dev).synchronize()
            return tuple(t.cpu().numpy() for t in out)
        return out


def plan_host(members, na, capacity, loaded=None, lib=None):
    """The assignment's plan as the device builds it, on the host: (order [E * na] call rows by member, tiles [T, 3] {member, p0, p1} =
    rows order[p0:p1], first bad env or -1)."""
    lib = lib or load_library()
    m = np.ascontiguousarray(np.asarray(members).reshape(-1), dtype=np.int32)
    E = m.size
    mt = C.c_int64()
    lib.check(lib.ac_policy_pool_max_tiles(E, int(na), int(capacity), C.byref(mt)), "ac_policy_pool_max_tiles")
    order = np.full(E * int(na), -1, dtype=np.int32)
    tiles = np.zeros((max(int(mt.value), 1), 3), dtype=np.int32)
    ld = None if loaded is None else np.ascontiguousarray(np.asarray(loaded).reshape(-1), dtype=np.int32)
    if ld is not None and ld.size != int(capacity):
        raise ValueError("plan_host: loaded must have capacity entries")
    nt, bad = C.c_int32(), C.c_int32()
    lib.check(lib.ac_policy_pool_plan_host(m.ctypes.data, E, int(na), int(capacity), None if ld is None else ld.ctypes.data, order.ctypes.data,
                                           tiles.ctypes.data, C.byref(nt), C.byref(bad)), "ac_policy_pool_plan_host")
    return order, tiles[:nt.value].copy(), int(bad.value)


def pool_compatible(pool_cfg, pool_form, cfg, form, lib=None):
    """None when a policy of (cfg, form) may be copied into a pool of (pool_cfg, pool_form) (forms "ppo" / "mappo"), else the reason."""
    lib = lib or load_library()
    f = lambda s: AC_POOL_MAPPO if s == "mappo" else AC_POOL_PPO
    return None if lib.ac_policy_pool_compatible(C.byref(pool_cfg), f(pool_form), C.byref(cfg), f(form)) == 0 else lib.last_error()
