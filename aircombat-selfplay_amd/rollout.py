"""A whole rollout of the reference's runners queued on the device in one call (include/aircombat_rollout.h for the PPO runners,
include/aircombat_rollout_share.h for the MAPPO share runner).

``DeviceRollout`` ties a ``HipVecEnv``, a ``DevicePolicy`` (with a critic), a ``DeviceReplayBuffer`` and, for self-play, an actor-only
``DevicePolicy`` or a ``DevicePolicyPool`` together. ``collect(n)`` then queues n steps of the runners' loop -- ``collect()``, the env
step and ``insert()`` of runner/jsbsim_runner.py:106-133 and runner/selfplay_jsbsim_runner.py:74-124 -- from C++ and returns without
waiting: per step the learner's launch on the buffer's slot, the opponent's launch, the env's step kernel(s) and one post-step kernel
that does what ``insert`` and ``ReplayBuffer.insert`` do (csrc/rollout_collect.hpp). The results are bit for bit those of the stepwise
loop of INTEGRATION.md §5d on the same handles.

Everything runs on the env's stream, ordered on the device after the work already queued on the caller's stream and the buffer's, and
before whatever is queued on either afterwards.

``DeviceMAPPORollout`` is the same for runner/share_jsbsim_runner.py: a ``HipShareVecEnv`` (or ``HipVecEnv``), a ``DeviceMAPPOPolicy``,
a ``DeviceSharedReplayBuffer`` and, for self-play, an actor-only ``DeviceMAPPOPolicy`` or a ``DevicePolicyPool(form="mappo")``. Its
post-step kernel (the same file's share form) also writes ``share_obs``, ``active_masks`` and the log-probs once per head column;
the results are bit for bit those of the stepwise loop of INTEGRATION.md §5e.

Out of scope for both: the per-step ``infos`` history, ``MultiDeviceVecEnv`` (one collector per device) and graph capture. The
mutual-support ``Discriminator`` of the MAPPO form needs no hook here: its intrinsic rewards are one launch after ``collect()``
(``DeviceDiscriminator.intrinsic_rewards``).
"""
import ctypes as C

from .capi import AcRolloutConfig, AC_ROLLOUT_NO_OPPONENT, AC_ROLLOUT_OPPONENT_POLICY, AC_ROLLOUT_OPPONENT_POOL
from .policy import DevicePolicy, DevicePolicyPool, HID

_U64 = 2 ** 64 - 1


def device_view(ptr, shape, device_id, typestr="<f4"):
    """torch view of device memory a collector or evaluator owns: ``shape`` elements of ``typestr`` at ``ptr`` on ``cuda:device_id``."""
    import torch
    holder = type("_View", (), {})()
    holder.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(holder, device=f"cuda:{device_id}")


def stream_of(device_id, stream):
    """(torch stream object, raw handle) of ``stream``: a ``torch.cuda.Stream``, a raw ``hipStream_t`` value, or None = torch's current."""
    import torch
    dev = torch.device("cuda", device_id)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    elif not hasattr(stream, "cuda_stream"):
        stream = torch.cuda.default_stream(dev) if int(stream) == 0 else torch.cuda.ExternalStream(int(stream), device=dev)
    return stream, stream.cuda_stream


def opponent_kind(opponent, num_learner_agents, num_agents, accepted):
    """(opponent kind of the C ABI, learner agents) for a collector or evaluator: the kind from ``opponent``'s type (the AC_ROLLOUT_* and
    AC_EVAL_* kinds are the same numbers), the learner's agents defaulting to all of them without an opponent and the first half with
    one. ``accepted`` words the ``TypeError`` for anything else."""
    if opponent is None:
        kind = AC_ROLLOUT_NO_OPPONENT
    elif isinstance(opponent, DevicePolicyPool):
        kind = AC_ROLLOUT_OPPONENT_POOL
    elif isinstance(opponent, DevicePolicy):
        kind = AC_ROLLOUT_OPPONENT_POLICY
    else:
        raise TypeError(f"opponent is None, {accepted}")
    if num_learner_agents is None:
        num_learner_agents = num_agents if opponent is None else num_agents // 2
    return kind, int(num_learner_agents)


class DeviceRollout:
    """``DeviceRollout(envs, policy, buffer, opponent=None, num_learner_agents=None)``: the learner ``policy`` owns agents
    ``[0, num_learner_agents)`` of every env (default: all of them without an opponent, the first half with one) and ``buffer`` holds
    their columns; ``opponent`` acts for the others. ``deterministic`` / ``opponent_deterministic`` pick the mode instead of drawing.
    The buffer's slot at ``buffer.step`` must hold the observations the env is about to act on (``buffer.set_slot("obs", 0, obs)`` after
    a reset; ``after_update`` carries them over). The handles must stay open while the collector is. A refusal (sizes, devices or forms
    that do not fit, a range past the buffer's end) raises ``ValueError`` and changes nothing."""

    _abi = "ac_rollout"            # prefix of the C functions: create, destroy, opponent_state, collect
    _opponent_doc = "a DevicePolicy(critic=False) or a DevicePolicyPool"

    def _c(self, name):
        return getattr(self.lib, f"{self._abi}_{name}")

    def __init__(self, envs, policy, buffer, opponent=None, num_learner_agents=None, deterministic=False, opponent_deterministic=False):
        self.lib = envs.lib
        self.envs, self.policy, self.buffer, self.opponent = envs, policy, buffer, opponent
        A = envs.num_agents
        kind, self.num_learner_agents = opponent_kind(opponent, num_learner_agents, A, self._opponent_doc)
        self.device_id = int(policy.device_id)
        cfg = AcRolloutConfig(self.num_learner_agents, kind, int(bool(deterministic)), int(bool(opponent_deterministic)))
        h = C.c_void_p()
        self._h = None
        if self._c("create")(envs._h, policy._h, buffer._h, None if opponent is None else opponent._h, C.byref(cfg), C.byref(h)) != 0:
            raise ValueError(self.lib.last_error())
        self._h = h
        self._opp_rows = envs.num_envs * (A - self.num_learner_agents)

    def close(self):
        if getattr(self, "_h", None):
            self._c("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _opponent_view(self, which):
        if self.opponent is None:
            return None
        h, m = C.c_void_p(), C.c_void_p()
        self.lib.check(self._c("opponent_state")(self._h, C.byref(h), C.byref(m)), f"{self._abi}_opponent_state")
        n = self._opp_rows
        shape, ptr = ((n, 1, HID), h) if which == 0 else ((n, 1), m)
        return device_view(ptr.value, shape, self.device_id)

    @property
    def opponent_states(self):
        """torch view [E * (A - na), 1, 128] of the opponent's GRU states (the collector owns them; None without an opponent)."""
        return self._opponent_view(0)

    @property
    def opponent_masks(self):
        """torch view [E * (A - na), 1] of the opponent's masks."""
        return self._opponent_view(1)

    def _stream(self, stream):
        return stream_of(self.device_id, stream)

    def collect(self, n_steps=None, stream=None):
        """Queue ``n_steps`` steps (default: the rest of the buffer) starting at ``buffer.step`` and return without waiting. ``stream``
        (a ``torch.cuda.Stream``, a raw ``hipStream_t`` value; default torch's current stream) is ordered around the rollout as the
        module docstring says; what the rollout reads must have been queued on it (or be complete) before the call: the weights of
        ``load_from_torch``, a pool's ``assign(check=False)``, slot 0's observations. Step t draws with ``policy.counter + t`` (the
        opponent with its own); both counters advance by ``n_steps``, so ``collect`` mixes with ``get_actions`` / ``act_into_env``
        calls in one stream of draws. Returns ``n_steps``. Should the runtime refuse a launch part of the way (after the refusals
        above have passed), the counters advance by the steps that were queued, as the buffer's step index does, before the error is
        raised."""
        T = self.buffer.buffer_size
        before = self.buffer.step
        if n_steps is None:
            n_steps = T - before
        n_steps = int(n_steps)
        tstream, raw = self._stream(stream)
        opp = self.opponent
        rc = self._c("collect")(self._h, raw, n_steps, C.c_uint64(self.policy.seed & _U64), C.c_uint64(self.policy.counter & _U64),
                                C.c_uint64((opp.seed if opp is not None else 0) & _U64),
                                C.c_uint64((opp.counter if opp is not None else 0) & _U64))
        done = n_steps if rc == 0 else (self.buffer.step - before) % T
        self.policy.counter += done
        if opp is not None:
            opp.counter += done
        if done:
            self._last_stream = tstream
        if rc != 0:
            raise ValueError(self.lib.last_error())
        return n_steps

    def compute_returns(self, wait=True):
        """The runners' ``compute()``, which ends a rollout and waits for it: ``policy.get_values`` on the buffer's last slot, queued on
        the stream the last ``collect`` was given (which that call ordered after the rollout), then
        ``buffer.compute_returns(next_values, on_device=True)``, which is a blocking call of the buffer's. Returns ``next_values``.

        ``wait=False`` queues both on that stream and returns without a ``synchronize``: ``get_values`` and
        ``buffer.compute_returns(next_values, on_device=True, wait=False)``. The returns (and ``next_values``) are there when the stream
        gets there; ``buffer.epoch`` or ``DevicePPOTrainer.train(..., stream_ordered=True)`` on the same stream follow without a wait."""
        import torch
        b, T = self.buffer, self.buffer.buffer_size
        stream = getattr(self, "_last_stream", None) or torch.cuda.current_stream(torch.device("cuda", self.device_id))
        with torch.cuda.stream(stream):
            next_values = self.policy.get_values(self._critic_input(T), b.device_tensor("rnn_states_critic")[T], b.device_tensor("masks")[T])
            if not wait:
                b.compute_returns(next_values, on_device=True, wait=False)
                return next_values
        stream.synchronize()   # the buffer copies next_values on its own stream
        b.compute_returns(next_values, on_device=True)
        return next_values

    def _critic_input(self, t):
        """the critic's input rows of buffer slot ``t``"""
        return self.buffer.device_tensor("obs")[t].reshape(-1, self.policy.obs_dim)


class DeviceMAPPORollout(DeviceRollout):
    """``DeviceMAPPORollout(envs, policy, buffer, opponent=None, num_learner_agents=None)``: ``DeviceRollout`` for the share runner
    (runner/share_jsbsim_runner.py). ``envs`` is a ``HipShareVecEnv`` or a ``HipVecEnv`` (only the handle is used), ``policy`` a
    ``DeviceMAPPOPolicy`` whose critic is ``num_agents * obs_dim`` wide, ``buffer`` a ``DeviceSharedReplayBuffer`` and ``opponent`` None,
    a ``DeviceMAPPOPolicy(critic=False)`` or a ``DevicePolicyPool(form="mappo")``. The buffer's slot at ``buffer.step`` must hold the
    observations and the share observations the env is about to act on (``set_slot("obs", 0, obs[:, :na])`` and
    ``set_slot("share_obs", 0, share_obs[:, :na])`` after a reset). ``collect``, ``compute_returns`` (``get_values`` on ``share_obs`` of the
    last slot), ``opponent_states``, ``opponent_masks`` and ``close`` are ``DeviceRollout``'s."""

    _abi = "ac_share_rollout"
    _opponent_doc = "a DeviceMAPPOPolicy(critic=False) or a DevicePolicyPool(form=\"mappo\")"

    def _critic_input(self, t):
        return self.buffer.device_tensor("share_obs")[t].reshape(-1, self.policy.cent_obs_dim)
