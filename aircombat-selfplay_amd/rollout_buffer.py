"""Device-resident rollout buffers behind the reference's buffer interface.

``DeviceReplayBuffer`` / ``DeviceSharedReplayBuffer`` mirror ``ReplayBuffer`` / ``SharedReplayBuffer`` of the reference
(algorithms/utils/buffer.py:26-268, :270-448): same constructor arguments, same method names, same argument meaning and the same
array layouts, but every array lives in HBM behind ``include/aircombat_buffer.h`` (``libaircombat_hip.so``). ``insert`` takes
numpy arrays (the reference's call, runner/jsbsim_runner.py:133) or device pointers / torch tensors on the buffer's GPU
(the env handle's own output buffers: no host round trip); ``compute_returns`` runs the reference's float32 recurrence as a HIP
kernel and is bit-identical to the numpy code; ``recurrent_generator`` gathers each mini-batch on the device.

Those calls block. ``compute_returns(..., wait=False)``, ``queue_advantages()`` and ``epoch(...)`` (a ``DeviceEpoch``: every mini-batch
of an epoch from one launch) are their stream-ordered forms behind ``include/aircombat_epoch.h``: queued on torch's current stream,
nothing waited for on the host.

There is no CPU implementation here: without the HIP library the constructor raises ``HipExtensionMissing``.
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import (AcBufferBatch, AcBufferConfig, AcBufferStep, AC_EPOCH_FIELDS, AC_EPOCH_NFIELDS, AC_BUF_ACTIONS, AC_BUF_ACTIVE_MASKS, AC_BUF_ADVANTAGES, AC_BUF_BAD_MASKS,
                   AC_BUF_LOGP, AC_BUF_MASKS, AC_BUF_OBS, AC_BUF_RETURNS, AC_BUF_REWARDS, AC_BUF_RNN_ACTOR, AC_BUF_RNN_CRITIC,
                   AC_BUF_SHARE_OBS, AC_BUF_VALUES)


def shape_from_space(space):
    """get_shape_from_space (algorithms/utils/utils.py:15-34) for gymnasium spaces or the stand-ins of vec_env.py; a plain int
    is taken as the flat dimension."""
    if isinstance(space, (int, np.integer)):
        return (int(space),)
    if isinstance(space, tuple) and len(space) == 2:          # Tuple(MultiDiscrete, Discrete | MultiDiscrete)
        second = space[1]
        return (len(space[0].nvec) + (len(second.nvec) if hasattr(second, "nvec") else 1),)
    if hasattr(space, "nvec") or (hasattr(space, "shape") and tuple(space.shape)):
        return tuple(space.shape)
    if hasattr(space, "n"):                                   # Discrete
        return (1,)
    raise NotImplementedError(f"Unsupported space type: {type(space)}!")


def _host(x):
    return np.ascontiguousarray(np.asarray(x), dtype=np.float32)


class DeviceEpoch:
    """The mini-batches of one epoch (``buffer.epoch(...)``), gathered by one launch into one flat float32 tensor on the buffer's GPU.
    ``len(epoch)`` mini-batches; ``epoch[i]`` (and iteration) gives the tuple ``minibatch(..., on_device=True)`` returns for
    ``order[i * mb:(i + 1) * mb]``: 9 entries for the PPO buffer, 11 for the shared one, same names, order, shapes and dtype, as views
    into ``flat``, which they keep alive. ``order`` is the device int32 tensor of the ``len(epoch) * mb`` chunk indices used. Everything is
    queued on the stream that was current when the epoch was made: read it on that stream, or after waiting for it."""

    def __init__(self, flat, order, batches, names):
        self.flat, self.order, self.names = flat, order, names
        self._batches = batches

    def __len__(self):
        return len(self._batches)

    def __getitem__(self, i):
        return self._batches[i]

    def __iter__(self):
        return iter(self._batches)


class DeviceReplayBuffer:
    """ReplayBuffer(args, num_agents, obs_space, act_space) (buffer.py:36-69). ``args`` needs buffer_size, n_rollout_threads,
    gamma, use_proper_time_limits, use_gae, gae_lambda, recurrent_hidden_size, recurrent_hidden_layers."""

    _shared = False
    FIELDS = {"obs": AC_BUF_OBS, "share_obs": AC_BUF_SHARE_OBS, "actions": AC_BUF_ACTIONS, "rewards": AC_BUF_REWARDS, "masks": AC_BUF_MASKS,
              "bad_masks": AC_BUF_BAD_MASKS, "active_masks": AC_BUF_ACTIVE_MASKS, "action_log_probs": AC_BUF_LOGP, "value_preds": AC_BUF_VALUES,
              "returns": AC_BUF_RETURNS, "rnn_states_actor": AC_BUF_RNN_ACTOR, "rnn_states_critic": AC_BUF_RNN_CRITIC}

    def __init__(self, args, num_agents, obs_space, act_space, share_obs_space=None, device_id=0):
        self.lib = capi.load_library()
        self.buffer_size, self.n_rollout_threads, self.num_agents = int(args.buffer_size), int(args.n_rollout_threads), int(num_agents)
        self.gamma, self.gae_lambda = float(args.gamma), float(args.gae_lambda)
        self.use_gae, self.use_proper_time_limits = bool(args.use_gae), bool(args.use_proper_time_limits)
        self.recurrent_hidden_size, self.recurrent_hidden_layers = int(args.recurrent_hidden_size), int(args.recurrent_hidden_layers)
        self.obs_shape, self.act_shape = shape_from_space(obs_space), shape_from_space(act_space)
        self.share_obs_shape = shape_from_space(share_obs_space) if self._shared else None
        cfg = AcBufferConfig(self.buffer_size, self.n_rollout_threads, self.num_agents, int(np.prod(self.obs_shape)),
                             int(np.prod(self.share_obs_shape)) if self._shared else 0, int(np.prod(self.act_shape)),
                             int(np.prod(self.act_shape)) if self._shared else 1, self.recurrent_hidden_layers, self.recurrent_hidden_size,
                             int(self.use_gae), int(self.use_proper_time_limits), self.gamma, self.gae_lambda)
        self._h = self.lib.ac_buffer_create(C.byref(cfg), int(device_id))
        if not self._h:
            raise RuntimeError(f"ac_buffer_create failed: {self.lib.last_error()}")
        self.device_id = int(device_id)
        T, E, A = self.buffer_size, self.n_rollout_threads, self.num_agents
        hid = (self.recurrent_hidden_layers, self.recurrent_hidden_size)
        self._shapes = {"obs": (T + 1, E, A) + self.obs_shape, "actions": (T, E, A) + self.act_shape, "rewards": (T, E, A, 1),
                        "masks": (T + 1, E, A, 1), "bad_masks": (T + 1, E, A, 1),
                        "action_log_probs": (T, E, A) + (self.act_shape if self._shared else (1,)),
                        "value_preds": (T + 1, E, A, 1), "returns": (T + 1, E, A, 1),
                        "rnn_states_actor": (T + 1, E, A) + hid, "rnn_states_critic": (T + 1, E, A) + hid}
        if self._shared:
            self._shapes.update(share_obs=(T + 1, E, A) + self.share_obs_shape, active_masks=(T + 1, E, A, 1))

    # ---- plumbing
    def close(self):
        if getattr(self, "_h", None):
            self.lib.ac_buffer_destroy(self._h)
            self._h = None

    __del__ = close

    def _ok(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {self.lib.last_error()}")

    @property
    def step(self):
        return self.lib.ac_buffer_step_index(self._h)

    def array(self, name):
        """Host copy of a whole array in the reference's shape (tests, logging); the training path never needs it."""
        fld = AC_BUF_ADVANTAGES if name == "advantages" else self.FIELDS[name]
        shape = (self.buffer_size, self.n_rollout_threads, self.num_agents, 1) if name == "advantages" else self._shapes[name]
        out = np.empty(shape, dtype=np.float32)
        self._ok(self.lib.ac_buffer_read(self._h, fld, out.ctypes.data), "ac_buffer_read")
        return out

    def set_slot(self, name, t, value):
        """buffer.<name>[t] = value (what the runners do once after reset: buffer.obs[0] = obs, runner/jsbsim_runner.py:36-42)."""
        v = _host(value)
        assert v.shape == self._shapes[name][1:], (v.shape, self._shapes[name][1:])
        self._ok(self.lib.ac_buffer_write_slot(self._h, self.FIELDS[name], int(t) % self._shapes[name][0], v.ctypes.data), "ac_buffer_write_slot")

    def device_tensor(self, name):
        """torch view of an array in HBM (no copy); requires torch with the ROCm runtime of the same process."""
        import torch
        fld = AC_BUF_ADVANTAGES if name == "advantages" else self.FIELDS[name]
        ptr, n = C.c_void_p(), C.c_int64()
        self._ok(self.lib.ac_buffer_device_ptr(self._h, fld, C.byref(ptr), C.byref(n)), "ac_buffer_device_ptr")
        shape = (self.buffer_size, self.n_rollout_threads, self.num_agents, 1) if name == "advantages" else self._shapes[name]
        iface = {"shape": (n.value,), "typestr": "<f4", "data": (ptr.value, False), "version": 2}
        holder = type("_View", (), {"__cuda_array_interface__": iface})()
        return torch.as_tensor(holder, device=f"cuda:{self.device_id}").view(shape)

    # ---- the reference's methods
    def insert(self, obs, actions, rewards, masks, action_log_probs, value_preds, rnn_states_actor, rnn_states_critic,
               bad_masks=None, share_obs=None, active_masks=None, available_actions=None, on_device=False, **kwargs):
        """buffer.py:77-111 / :313-343. With on_device=True every argument is a device pointer (int) or a torch tensor on the
        buffer's GPU holding contiguous float32."""
        keep = []

        def ptr(x):
            if x is None:
                return None
            if on_device:
                return int(x) if isinstance(x, (int, np.integer)) else int(x.data_ptr())
            a = _host(x)
            keep.append(a)
            return a.ctypes.data
        step = AcBufferStep(ptr(obs), ptr(actions), ptr(rewards), ptr(masks), ptr(action_log_probs), ptr(value_preds), ptr(rnn_states_actor),
                            ptr(rnn_states_critic), ptr(bad_masks), ptr(share_obs), ptr(active_masks))
        self._ok(self.lib.ac_buffer_insert(self._h, C.byref(step), int(on_device)), "ac_buffer_insert")

    def after_update(self):
        self._ok(self.lib.ac_buffer_after_update(self._h), "ac_buffer_after_update")

    def clear(self):
        self._ok(self.lib.ac_buffer_clear(self._h), "ac_buffer_clear")

    def _current_stream(self):
        import torch
        return torch.cuda.current_stream(torch.device("cuda", self.device_id)).cuda_stream

    def compute_returns(self, next_value, on_device=False, wait=True):
        """buffer.py:134-167. ``wait=False`` (with ``on_device=True`` only: a host array could be reused before it is read) queues the
        same copy and the same kernel on torch's current stream and returns at once; ``next_value`` must have been produced on that
        stream (or be complete), and ``last_returns_kernel_ms`` is not updated."""
        if not wait:
            if not on_device:
                raise ValueError("compute_returns: wait=False takes a device next_value (on_device=True)")
            p = int(next_value) if isinstance(next_value, (int, np.integer)) else int(next_value.data_ptr())
            self._ok(self.lib.ac_buffer_compute_returns_on(self._h, self._current_stream(), p), "ac_buffer_compute_returns_on")
        elif on_device:
            p = int(next_value) if isinstance(next_value, (int, np.integer)) else int(next_value.data_ptr())
            self._ok(self.lib.ac_buffer_compute_returns(self._h, p, 1), "ac_buffer_compute_returns")
        else:
            v = _host(next_value)
            assert v.size == self.n_rollout_threads * self.num_agents
            self._ok(self.lib.ac_buffer_compute_returns(self._h, v.ctypes.data, 0), "ac_buffer_compute_returns")

    def last_returns_kernel_ms(self):
        ms = C.c_float()
        self._ok(self.lib.ac_buffer_last_kernel_ms(self._h, C.byref(ms)), "ac_buffer_last_kernel_ms")
        return ms.value

    @property
    def advantages(self):
        """buffer.py:72-75 (host copy; the generator below reads the device array)."""
        self._ok(self.lib.ac_buffer_advantages(self._h), "ac_buffer_advantages")
        return self.array("advantages")

    def queue_advantages(self):
        """The ``advantages`` property's three kernels queued on torch's current stream, nothing waited for and nothing returned: the
        normalised advantages are in ``device_tensor("advantages")`` when the stream gets there."""
        self._ok(self.lib.ac_buffer_advantages_on(self._h, self._current_stream()), "ac_buffer_advantages_on")

    # names of the per-step arrays of a mini-batch, in the order the reference yields them
    _BATCH = ("obs", "actions", "masks", "action_log_probs", "advantages", "returns", "value_preds")

    def minibatch(self, chunks, data_chunk_length, on_device=False):
        """One mini-batch for the given chunk indices (host numpy arrays in the reference's order and shapes). With on_device=True
        the same arrays, bit for bit, as float32 torch tensors on the buffer's GPU, gathered in HBM (no copy across PCIe).

        The gather runs on the buffer's own stream. Torch's caching allocator may hand out memory that work queued on torch's
        current stream still reads, so that stream is waited for first; the gather then ends with a wait for the buffer's stream,
        and the tensors are complete, safe to read on any stream, when they are returned."""
        return self._minibatch([self], chunks, data_chunk_length, on_device)

    def _minibatch(self, buffers, chunks, data_chunk_length, on_device):
        """``minibatch`` for chunk indices into the stack of ``buffers`` (``self`` is its first): ``[self]`` goes through the
        single-handle call, a longer list through the list call."""
        chunks = np.ascontiguousarray(chunks, dtype=np.int32)
        n, L = len(chunks), int(data_chunk_length)
        widths = {"obs": self.obs_shape, "share_obs": self.share_obs_shape, "actions": self.act_shape, "masks": (1,), "active_masks": (1,),
                  "action_log_probs": self._shapes["action_log_probs"][3:], "advantages": (1,), "returns": (1,), "value_preds": (1,)}
        shapes = {k: (L * n,) + tuple(widths[k]) for k in self._BATCH}
        hid = (self.recurrent_hidden_layers, self.recurrent_hidden_size)
        shapes["rnn_states_actor"], shapes["rnn_states_critic"] = (n,) + hid, (n,) + hid
        if on_device:
            import torch
            dev = torch.device("cuda", self.device_id)
            outs = {k: torch.empty(s, dtype=torch.float32, device=dev) for k, s in shapes.items()}
            torch.cuda.current_stream(dev).synchronize()
            batch = AcBufferBatch(**{k: v.data_ptr() for k, v in outs.items()})
        else:
            outs = {k: np.empty(s, dtype=np.float32) for k, s in shapes.items()}
            batch = AcBufferBatch(**{k: v.ctypes.data for k, v in outs.items()})
        if len(buffers) == 1:
            self._ok(self.lib.ac_buffer_minibatch(self._h, chunks.ctypes.data, n, L, C.byref(batch), int(bool(on_device))), "ac_buffer_minibatch")
        else:
            self._ok(self.lib.ac_buffers_minibatch(_handles(buffers), len(buffers), chunks.ctypes.data, n, L, C.byref(batch), int(bool(on_device))),
                     "ac_buffers_minibatch")
        return tuple(outs[k] for k in self._BATCH) + (outs["rnn_states_actor"], outs["rnn_states_critic"])

    @staticmethod
    def epoch_of(buffers, num_mini_batch, data_chunk_length, chunk_order=None):
        """``epoch`` over a list of up to 8 device buffers of one shape, as the reference's ``recurrent_generator`` treats a list of
        buffers (buffer.py:183-214): the buffers' sequence views are stacked in the list's order and one chunk order runs over the
        stack, ``data_chunks = n_rollout_threads * (buffer_size * K) // data_chunk_length`` chunks (the reference's formula: the agent
        axis is not counted), so every mini-batch mixes rows of every buffer and a chunk may straddle two of them. One flat tensor,
        ``queue_advantages()`` on every buffer (each buffer's advantages are normalised on its own, as the reference does) and then ONE
        gather launch, all on torch's current stream with nothing waited for. ``chunk_order`` is ``epoch``'s, its indices chunks of
        the stack. A list of one buffer gives ``buffer.epoch(...)`` bit for bit.

        A list of ``DeviceSharedReplayBuffer`` is taken the same way: the reference's MAPPO generator has no list form, so this is the
        PPO list rule applied to the shared buffer's fields (``share_obs`` and ``active_masks`` are stacked like ``obs`` and ``masks``).
        ``ValueError`` for anything in the list that is no device buffer; buffers that differ in shape, class or device, the same
        buffer twice and more than 8 buffers are refused by the library with the cause named, before anything is queued."""
        buffers = _buffer_list(buffers, "epoch_of")
        return buffers[0]._epoch(buffers, num_mini_batch, data_chunk_length, chunk_order, True)

    def epoch(self, num_mini_batch, data_chunk_length, chunk_order=None):
        """Every mini-batch of one pass of ``recurrent_generator(..., on_device=True)`` as a ``DeviceEpoch``, without a host wait: one
        flat tensor from torch's allocator (safe without a wait: everything here runs on torch's current stream), the advantages
        (``queue_advantages``) and ONE gather launch for all fields of all mini-batches. The number of chunks, the mini-batch size and
        the dropped remainder are ``recurrent_generator``'s: ``data_chunks = n_rollout_threads * buffer_size // data_chunk_length``,
        ``mb = data_chunks // num_mini_batch``, and the chunks past ``num_mini_batch * mb`` of the order are not used.

        ``chunk_order=None`` draws ``torch.randperm(data_chunks, device=...)`` ON THE DEVICE, i.e. from torch's device generator and
        not from the CPU generator the reference and ``recurrent_generator`` draw from: under one ``torch.manual_seed`` the two give
        different (equally uniform) permutations. A host array (numpy, list, CPU tensor) is checked on the host exactly as
        ``minibatch`` checks its chunks and sent through pinned memory without blocking. An integer tensor on the buffer's GPU is
        used as it is, unchecked: the kernel clamps every index into the valid range, which keeps a bad index from reading
        outside the buffer but does not report it."""
        return self._epoch([self], num_mini_batch, data_chunk_length, chunk_order, False)

    def _epoch(self, buffers, num_mini_batch, data_chunk_length, chunk_order, as_list):
        """``epoch`` (the single-handle calls) or, ``as_list``, ``epoch_of`` (the list calls) over ``buffers``, whose first is ``self``."""
        import torch
        K = len(buffers)
        n_mb, L = int(num_mini_batch), int(data_chunk_length)
        assert self.n_rollout_threads * self.buffer_size * K >= L, "PPO requires n_rollout_threads * buffer_size >= data_chunk_length"
        data_chunks = self.n_rollout_threads * (self.buffer_size * K) // L
        mb = data_chunks // n_mb
        if n_mb < 1 or mb < 1:
            raise ValueError(f"epoch: {data_chunks} chunks do not fill {n_mb} mini-batches")
        dev, used = torch.device("cuda", self.device_id), n_mb * mb
        offsets, total = (C.c_int64 * AC_EPOCH_NFIELDS)(), C.c_int64()
        if as_list:   # the list's refusals (shapes, classes, devices, a handle twice) come before anything is drawn or queued
            handles = _handles(buffers)
            self._ok(self.lib.ac_buffers_epoch_layout(handles, K, n_mb, mb, L, offsets, C.byref(total)), "ac_buffers_epoch_layout")
        with torch.cuda.device(dev):
            if chunk_order is None:
                order = torch.randperm(data_chunks, device=dev)[:used].to(torch.int32)
            elif isinstance(chunk_order, torch.Tensor) and chunk_order.device.type == "cuda":
                if chunk_order.device != dev or chunk_order.dtype.is_floating_point or chunk_order.dtype == torch.bool or chunk_order.numel() < used:
                    raise ValueError(f"epoch: chunk_order must be an integer tensor of at least {used} indices on {dev}")
                order = chunk_order.reshape(-1)[:used].to(torch.int32).contiguous()
            else:
                host = np.ascontiguousarray(np.asarray(chunk_order).reshape(-1)[:used], dtype=np.int32)
                if host.size < used:
                    raise ValueError(f"epoch: chunk_order holds {host.size} indices, {used} are needed")
                rows = self.buffer_size * K * self.n_rollout_threads * self.num_agents
                if (host < 0).any() or ((host.astype(np.int64) + 1) * L > rows).any():
                    raise RuntimeError("epoch failed: chunk index outside the buffer")
                pinned = torch.empty(used, dtype=torch.int32, pin_memory=True)
                pinned.numpy()[:] = host
                order = pinned.to(dev, non_blocking=True)   # torch's host allocator orders the reuse of `pinned` after the copy
            if not as_list:
                self._ok(self.lib.ac_buffer_epoch_layout(self._h, n_mb, mb, L, offsets, C.byref(total)), "ac_buffer_epoch_layout")
            flat = torch.empty(total.value, dtype=torch.float32, device=dev)
            for b in buffers:
                b.queue_advantages()
            if as_list:
                self._ok(self.lib.ac_buffers_gather_epoch(handles, K, self._current_stream(), order.data_ptr(), n_mb, mb, L, flat.data_ptr()),
                         "ac_buffers_gather_epoch")
            else:
                self._ok(self.lib.ac_buffer_gather_epoch(self._h, self._current_stream(), order.data_ptr(), n_mb, mb, L, flat.data_ptr()),
                         "ac_buffer_gather_epoch")
        widths = {"obs": self.obs_shape, "share_obs": self.share_obs_shape, "actions": self.act_shape, "masks": (1,), "active_masks": (1,),
                  "action_log_probs": self._shapes["action_log_probs"][3:], "advantages": (1,), "returns": (1,), "value_preds": (1,)}
        hid = (self.recurrent_hidden_layers, self.recurrent_hidden_size)
        names = self._BATCH + ("rnn_states_actor", "rnn_states_critic")
        batches = []
        for i in range(n_mb):
            item = []
            for k in names:
                shape = ((mb,) + hid) if k.startswith("rnn_states") else ((L * mb,) + tuple(widths[k]))
                n = int(np.prod(shape))
                at = offsets[AC_EPOCH_FIELDS.index(k)] + i * n
                item.append(flat[at:at + n].view(shape))
            batches.append(tuple(item))
        return DeviceEpoch(flat, order, batches, names)

    @staticmethod
    def recurrent_generator(buffer, num_mini_batch, data_chunk_length, chunk_order=None, on_device=False):
        """ReplayBuffer.recurrent_generator(buffer, num_mini_batch, data_chunk_length) (buffer.py:169-268): the chunk permutation
        comes from torch.randperm (the CPU generator) like the reference's unless ``chunk_order`` is given (tests). The number of
        chunks follows the reference: n_rollout_threads * buffer_size // data_chunk_length (the agent axis is not counted).
        on_device=True yields torch tensors on the buffer's GPU instead of numpy arrays (``minibatch``).

        ``buffer`` is one device buffer or, as in the reference, a list of up to 8 of one shape: their sequence views are stacked in
        the list's order (the reference's np.vstack), ``buffer_size`` counts K times in the number of chunks, each buffer's
        advantages are normalised on its own, and one permutation over the stack's chunks cuts mini-batches that mix rows of every
        buffer (a chunk may straddle two of them). A list of ``DeviceSharedReplayBuffer`` is taken the same way: the reference's MAPPO
        generator has no list form, so this is the PPO list rule applied to the shared buffer's fields. See ``epoch_of`` for what a
        list is refused for."""
        buffers = _buffer_list(buffer, "recurrent_generator")
        self, K = buffers[0], len(buffers)
        L, n_mb = int(data_chunk_length), int(num_mini_batch)
        assert self.n_rollout_threads * self.buffer_size * K >= L, "PPO requires n_rollout_threads * buffer_size >= data_chunk_length"
        data_chunks = self.n_rollout_threads * (self.buffer_size * K) // L
        mb = data_chunks // n_mb
        if K > 1:   # the list's refusals before anything runs
            offsets, total = (C.c_int64 * AC_EPOCH_NFIELDS)(), C.c_int64()
            self._ok(self.lib.ac_buffers_epoch_layout(_handles(buffers), K, n_mb, max(mb, 1), L, offsets, C.byref(total)), "ac_buffers_epoch_layout")
        if chunk_order is None:
            import torch
            chunk_order = torch.randperm(data_chunks).numpy()
        chunk_order = np.asarray(chunk_order)
        for b in buffers:
            b._ok(b.lib.ac_buffer_advantages(b._h), "ac_buffer_advantages")
        for i in range(n_mb):
            yield self._minibatch(buffers, chunk_order[i * mb:(i + 1) * mb], L, on_device)


def _buffer_list(buffers, what):
    """One device buffer or a list / tuple of them as a list; ValueError for an empty list or anything else in it (the reference's host
    buffers among them: they gather on the host)."""
    buffers = list(buffers) if isinstance(buffers, (list, tuple)) else [buffers]
    if not buffers or not all(isinstance(b, DeviceReplayBuffer) for b in buffers):
        raise ValueError(f"{what}: a DeviceReplayBuffer / DeviceSharedReplayBuffer or a list of them is needed, got "
                         f"[{', '.join(type(b).__name__ for b in buffers)}]")
    return buffers


def _handles(buffers):
    """The C array of the buffers' handles (a closed buffer's is NULL, which the library refuses)."""
    return (C.c_void_p * len(buffers))(*[b._h for b in buffers])


class DeviceSharedReplayBuffer(DeviceReplayBuffer):
    """SharedReplayBuffer(args, num_agents, obs_space, share_obs_space, act_space) (buffer.py:272-311)."""

    _shared = True
    _BATCH = ("obs", "share_obs", "actions", "masks", "active_masks", "action_log_probs", "advantages", "returns", "value_preds")

    def __init__(self, args, num_agents, obs_space, share_obs_space, act_space, device_id=0):
        super().__init__(args, num_agents, obs_space, act_space, share_obs_space=share_obs_space, device_id=device_id)

    def insert(self, obs, share_obs, actions, rewards, masks, action_log_probs, value_preds, rnn_states_actor, rnn_states_critic,
               bad_masks=None, active_masks=None, available_actions=None, on_device=False):
        return super().insert(obs, actions, rewards, masks, action_log_probs, value_preds, rnn_states_actor, rnn_states_critic,
                              bad_masks=bad_masks, share_obs=share_obs, active_masks=active_masks, on_device=on_device)

    def recurrent_generator(self, advantages, num_mini_batch, data_chunk_length, chunk_order=None, on_device=False):   # noqa: buffer.py:350
        """buffer.recurrent_generator(buffer.advantages, num_mini_batch, data_chunk_length) (mappo/ppo_trainer.py:90). The
        advantages argument is the buffer's own normalised advantages in the reference's only call; the device copy is used."""
        return DeviceReplayBuffer.recurrent_generator(self, num_mini_batch, data_chunk_length, chunk_order=chunk_order, on_device=on_device)
