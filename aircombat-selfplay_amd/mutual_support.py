"""The reference's mutual-support ``Discriminator`` (algorithms/utils/discriminator.py) with its hot paths on the device
(``include/aircombat_mutual.h``, ``csrc/mutual_support.hpp``).

Two three-layer nets predict an agent's next observation from agent 0's actor state entering the step and the actions of agents 0 and 1:
``pred`` with the partner's action, ``pred_wo`` without. The intrinsic reward of an agent is how much the partner's action helped,
``mse_wo - mse_with`` of the partner's tuple, as the reference's ``compute_MI`` scores it on the input layout ``update_parameters``
trains on (its ``compute_intrinsic_reward`` cannot run as written: it feeds ``pred`` 138 columns against a 142-column layer).

``DeviceDiscriminator.intrinsic_rewards(buffer)`` scores every step of a collected rollout in ONE launch that reads the buffer's arrays
and the torch parameters in place; ``train(buffer)`` gathers each mini-batch with one launch and keeps the dense products in torch.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .capi import AcMiGather, AcMiScore, AC_BUF_ACTIONS, AC_BUF_OBS, AC_BUF_REWARDS, AC_BUF_RNN_ACTOR, AC_MI_HIDDEN, AC_MI_MAX_ACT, AC_MI_MAX_OBS, AC_MI_WIDTH
from .policy import UnsupportedPolicy
from .ppo_update import device_clip_adam_step
from .rollout_buffer import DeviceSharedReplayBuffer, shape_from_space


def _act_columns(act_space):
    """Columns of an action row: the reference sums ``len(s.nvec)`` over a Tuple's parts; any other space counts as the buffer does."""
    parts = getattr(act_space, "spaces", None)
    if parts is None and isinstance(act_space, tuple):
        parts = act_space
    if parts is not None and all(hasattr(s, "nvec") for s in parts):
        return int(sum(len(s.nvec) for s in parts))
    return int(np.prod(shape_from_space(act_space)))


class PredictNet(nn.Module):
    """Linear - ReLU per hidden width, then a Linear head; the parameter names (``layers.<i>``, ``last_fc``) are the checkpoint's."""

    def __init__(self, input_dim, output_dim, widths):
        super().__init__()
        self.layers = nn.ModuleList()
        for w in widths:
            self.layers.append(nn.Linear(input_dim, w))
            input_dim = w
        self.last_fc = nn.Linear(input_dim, output_dim)

    def forward(self, x):
        for layer in self.layers:
            x = F.relu(layer(x))
        return self.last_fc(x)


class DeviceDiscriminator(nn.Module):
    """``Discriminator(args, num_agents, obs_space, share_obs_space, act_space, device)``: same arguments, same ``state_dict`` keys
    (``pred.layers.{0,1}.*``, ``pred.last_fc.*`` and the same under ``pred_wo``), ``q_optimizer`` (one Adam over both nets, ``args.lr``)
    and ``q_loss_coef``. ``args`` needs ppo_epoch, num_mini_batch, hidden_size, recurrent_hidden_size, lr; ``intrinsic_ratio`` is the
    default of ``intrinsic_rewards``'s ``ratio``.

    Accepted (anything else raises ``UnsupportedPolicy`` naming the value): 1 .. 12 action columns, an observation of 1 .. 128 values,
    ``hidden_size "128 128"`` (net widths 256 / 256) and ``recurrent_hidden_size`` 128. ``num_agents < 2`` is a ``ValueError``."""

    def __init__(self, args, num_agents, obs_space, share_obs_space, act_space, device=torch.device("cuda", 0)):
        super().__init__()
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.num_agents = int(num_agents)
        if self.num_agents < 2:
            raise ValueError(f"DeviceDiscriminator: num_agents {self.num_agents} is below 2 (the scores pair agents 0 and 1)")
        self.ppo_epoch, self.num_mini_batch = int(args.ppo_epoch), int(args.num_mini_batch)
        self.hidden_size = args.hidden_size
        self.data_chunk_length = getattr(args, "data_chunk_length", None)
        self.recurrent_hidden_size = int(args.recurrent_hidden_size)
        self.intrinsic_ratio = float(getattr(args, "intrinsic_ratio", 0.0))
        widths = [2 * int(w) for w in str(args.hidden_size).split()]
        self.act_dim = _act_columns(act_space)
        self.output_dim = int(shape_from_space(obs_space)[0])
        if widths != [AC_MI_WIDTH, AC_MI_WIDTH]:
            raise UnsupportedPolicy(f"DeviceDiscriminator: hidden_size {args.hidden_size!r} gives net widths {widths}, the scorer takes 256 / 256 ('128 128')")
        if self.recurrent_hidden_size != AC_MI_HIDDEN:
            raise UnsupportedPolicy(f"DeviceDiscriminator: recurrent_hidden_size {self.recurrent_hidden_size} is not 128")
        if not 1 <= self.act_dim <= AC_MI_MAX_ACT:
            raise UnsupportedPolicy(f"DeviceDiscriminator: {self.act_dim} action columns are outside 1 .. 12")
        if not 1 <= self.output_dim <= AC_MI_MAX_OBS:
            raise UnsupportedPolicy(f"DeviceDiscriminator: obs_dim {self.output_dim} is outside 1 .. 128")
        self.input_dim = 2 * self.act_dim + self.recurrent_hidden_size
        self.input_dim_wo_act = self.act_dim + self.recurrent_hidden_size
        self.pred = PredictNet(self.input_dim, self.output_dim, widths).to(dtype=torch.float32, device=self.device)
        self.pred_wo = PredictNet(self.input_dim_wo_act, self.output_dim, widths).to(dtype=torch.float32, device=self.device)
        self.q_optimizer = torch.optim.Adam(list(self.pred.parameters()) + list(self.pred_wo.parameters()), lr=args.lr)
        self.q_loss_coef = 0.01

    # ---- checks shared by the two device paths: everything is refused before anything is touched
    def _check_buffer(self, buffer, what):
        if not isinstance(buffer, DeviceSharedReplayBuffer):
            raise ValueError(f"{what}: a DeviceSharedReplayBuffer is needed, got {type(buffer).__name__}")
        if self.device.type != "cuda" or buffer.device_id != self.device.index:
            raise ValueError(f"{what}: the buffer is on cuda:{buffer.device_id}, the discriminator on {self.device}")
        if buffer.num_agents < 2:
            raise ValueError(f"{what}: the buffer has {buffer.num_agents} agent, two are needed")
        got = (buffer.num_agents, int(np.prod(buffer.obs_shape)), int(np.prod(buffer.act_shape)), buffer.recurrent_hidden_size, buffer.recurrent_hidden_layers)
        want = (self.num_agents, self.output_dim, self.act_dim, self.recurrent_hidden_size, 1)
        if got != want:
            raise ValueError(f"{what}: the buffer's (num_agents, obs_dim, act_dim, recurrent_hidden_size, recurrent_hidden_layers) = {got}, "
                             f"the discriminator's are {want}")

    def _check_parameters(self, what):
        for name, p in self.named_parameters():
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != self.device:
                raise ValueError(f"{what}: parameter {name} must be contiguous float32 on {self.device}")

    def _array(self, buffer, field):
        ptr, n = C.c_void_p(), C.c_int64()
        buffer._ok(buffer.lib.ac_buffer_device_ptr(buffer._h, field, C.byref(ptr), C.byref(n)), "ac_buffer_device_ptr")
        return ptr.value

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def intrinsic_rewards(self, buffer, start=0, n_steps=None, ratio=None, add=True):
        """The intrinsic rewards of steps ``[start, start + n_steps)`` of a collected rollout (default: all ``buffer_size`` steps): one
        launch on torch's current stream, no host wait. Returns ``r_int`` as a device tensor ``[n_steps, E, num_agents, 1]`` (agents >= 2
        get 0); with ``add=True`` it also adds ``ratio * r_int`` into the buffer's ``rewards`` (``ratio`` defaults to
        ``args.intrinsic_ratio``). Calling it twice with ``add=True`` adds twice: call it once per rollout, after ``collect()`` and
        before ``compute_returns``.

        The step's slots ``s`` and ``s + 1`` must already be written, by work queued on this stream or complete. What is queued on this
        stream afterwards sees the new rewards; the buffer's blocking calls run on its own stream, so synchronise this one first (as
        ``DeviceMAPPORollout.compute_returns()`` does)."""
        what = "intrinsic_rewards"
        self._check_buffer(buffer, what)
        T, E, A = buffer.buffer_size, buffer.n_rollout_threads, buffer.num_agents
        start = int(start)
        n = T - start if n_steps is None else int(n_steps)
        if start < 0 or n < 1 or start + n > T:
            raise ValueError(f"{what}: steps [{start}, {start + n}) are not inside the buffer's [0, {T})")
        self._check_parameters(what)
        ratio = self.intrinsic_ratio if ratio is None else float(ratio)
        lib = buffer.lib
        with torch.cuda.device(self.device):
            out = torch.zeros((n, E, A, 1), dtype=torch.float32, device=self.device)
            pair = out if A == 2 else torch.empty((n, E, 2), dtype=torch.float32, device=self.device)
            args = self._score_args(buffer, start, n, ratio, add, pair.data_ptr(), None)
            if lib.ac_mi_score(C.byref(args), self._stream()) != 0:
                raise RuntimeError(f"ac_mi_score failed: {lib.last_error()}")
            if A != 2:
                out[:, :, :2, 0] = pair
        return out

    def _score_args(self, buffer, start, n, ratio, add, r_int, mse):
        P, Q = self.pred, self.pred_wo
        w = [t.data_ptr() for net in (P, Q) for lin in (net.layers[0], net.layers[1], net.last_fc) for t in (lin.weight, lin.bias)]
        return AcMiScore(buffer.n_rollout_threads, buffer.num_agents, buffer.buffer_size, self.output_dim, self.act_dim, self.recurrent_hidden_size,
                         start, n, int(bool(add)), ratio, self._array(buffer, AC_BUF_OBS), self._array(buffer, AC_BUF_ACTIONS),
                         self._array(buffer, AC_BUF_RNN_ACTOR), self._array(buffer, AC_BUF_REWARDS), *w, r_int, mse)

    def step_mse(self, buffer, start=0, n_steps=None):
        """Diagnostics: the scorer's four mean squared errors per step and env as a device tensor ``[n, E, 2, 2]``, entry
        ``[.., j, 0]`` = mse_with(j), ``[.., j, 1]`` = mse_wo(j). Nothing is added to the buffer."""
        self._check_buffer(buffer, "step_mse")
        T, E = buffer.buffer_size, buffer.n_rollout_threads
        start = int(start)
        n = T - start if n_steps is None else int(n_steps)
        if start < 0 or n < 1 or start + n > T:
            raise ValueError(f"step_mse: steps [{start}, {start + n}) are not inside the buffer's [0, {T})")
        self._check_parameters("step_mse")
        with torch.cuda.device(self.device):
            mse = torch.empty((n, E, 2, 2), dtype=torch.float32, device=self.device)
            args = self._score_args(buffer, start, n, 0.0, False, None, mse.data_ptr())
            if buffer.lib.ac_mi_score(C.byref(args), self._stream()) != 0:
                raise RuntimeError(f"ac_mi_score failed: {buffer.lib.last_error()}")
        return mse

    def gather(self, buffer, times):
        """One mini-batch for the int32 device tensor ``times``: ``X [2 m E, 128 + 2 C]`` and ``Y [2 m E, obs_dim]``, tuple 0's rows then
        tuple 1's, from one launch on torch's current stream."""
        m, E = int(times.numel()), buffer.n_rollout_threads
        X = torch.empty((2 * m * E, self.input_dim), dtype=torch.float32, device=self.device)
        Y = torch.empty((2 * m * E, self.output_dim), dtype=torch.float32, device=self.device)
        args = AcMiGather(E, buffer.num_agents, buffer.buffer_size, self.output_dim, self.act_dim, self.recurrent_hidden_size, m, 0,
                          self._array(buffer, AC_BUF_OBS), self._array(buffer, AC_BUF_ACTIONS), self._array(buffer, AC_BUF_RNN_ACTOR),
                          times.data_ptr(), X.data_ptr(), Y.data_ptr())
        if buffer.lib.ac_mi_gather(C.byref(args), self._stream()) != 0:
            raise RuntimeError(f"ac_mi_gather failed: {buffer.lib.last_error()}")
        return X, Y

    def minibatch_loss(self, X, Y):
        """``update_parameters``'s loss on a gathered mini-batch: q_loss_coef * sum over the two tuples of the two nets' mean squared
        errors (the reference's per-thread sum divided by the thread count is this mean)."""
        half = X.shape[0] // 2
        with_act, without = self.pred(X), self.pred_wo(X[:, :self.input_dim_wo_act])
        loss = 0.0
        for rows in (slice(0, half), slice(half, 2 * half)):
            loss = loss + F.mse_loss(with_act[rows], Y[rows]) + F.mse_loss(without[rows], Y[rows])
        return self.q_loss_coef * loss

    def train(self, buffer=True, time_orders=None):
        """``Discriminator.train(buffer)``: ``ppo_epoch`` epochs of ``num_mini_batch`` mini-batches of ``T // num_mini_batch`` time
        indices each (a permutation of ``range(T)`` per epoch, the remainder dropped), all envs and both tuples in every mini-batch. Per
        mini-batch: the gather launch, the two nets forward and backward in torch, ``device_clip_adam_step`` for the Adam step. The
        losses collect in one device tensor (kept as ``last_losses``) that is read once at the end. Returns ``{"disc_loss": mean}``.

        ``time_orders``: ``ppo_epoch`` permutations of ``range(T)`` (reproducible tests); by default torch's DEVICE generator draws them,
        where the reference draws from the CPU generator. (A bool is ``nn.Module.train(mode)``, so ``eval()`` keeps working.)"""
        if isinstance(buffer, bool):
            return super().train(buffer)
        self._check_buffer(buffer, "train")
        T = buffer.buffer_size
        mb = T // self.num_mini_batch
        if mb < 1:
            raise ValueError(f"train: {T} steps do not fill {self.num_mini_batch} mini-batches")
        self._check_parameters("train")
        if time_orders is not None:
            time_orders = [np.asarray(o, dtype=np.int64).reshape(-1) for o in time_orders]
            if len(time_orders) != self.ppo_epoch or any(sorted(o.tolist()) != list(range(T)) for o in time_orders):
                raise ValueError(f"train: time_orders must be {self.ppo_epoch} permutations of range({T})")
        with torch.cuda.device(self.device):
            losses = torch.zeros(self.ppo_epoch * self.num_mini_batch, dtype=torch.float32, device=self.device)
            for ep in range(self.ppo_epoch):
                if time_orders is None:
                    order = torch.randperm(T, device=self.device).to(torch.int32)
                else:
                    order = torch.tensor(time_orders[ep], dtype=torch.int32, device=self.device)
                for i in range(self.num_mini_batch):
                    X, Y = self.gather(buffer, order[i * mb:(i + 1) * mb].contiguous())
                    loss = self.minibatch_loss(X, Y)
                    self.q_optimizer.zero_grad()
                    loss.backward()
                    device_clip_adam_step(self.q_optimizer, 0.0, clip=False)
                    losses[ep * self.num_mini_batch + i] = loss.detach()
            self.last_losses = losses      # the mini-batches' losses in order, a device tensor [ppo_epoch * num_mini_batch]
            return {"disc_loss": float(losses.mean())}

    @torch.no_grad()
    def compute_MI(self, obs, next_obs, actions, dones, rnn_states_actor):
        """The reference's per-env score for rendering: ``obs``, ``next_obs`` ``[agents, obs_dim]``, ``actions`` ``[agents, C]``,
        ``rnn_states_actor`` agent 0's state (any shape holding 128 values). Returns a numpy array ``[agents]``: entry 1 is tuple 0's
        score, entry 0 tuple 1's, the rest 0. Plain torch."""
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).to(self.device)
        next_obs, actions, h = t(next_obs), t(actions), t(rnn_states_actor).reshape(-1)
        out = torch.zeros(next_obs.shape[0], dtype=torch.float32, device=self.device)
        for j in (0, 1):
            x = torch.cat([h, actions[j], actions[1 - j]])
            with_act = F.mse_loss(self.pred(x), next_obs[j])
            without = F.mse_loss(self.pred_wo(x[:self.input_dim_wo_act]), next_obs[j])
            out[1 - j] = without - with_act
        return out.cpu().numpy()
