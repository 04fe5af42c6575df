"""The rest of the PPO / MAPPO update on the device ("The loss, the clip and Adam").

After ``policy.evaluate_actions`` the reference's ``PPOTrainer.ppo_update`` (algorithms/ppo/ppo_trainer.py:44-74, the same lines in
algorithms/mappo/ppo_trainer.py) runs the loss, ``clip_grad_norm_`` twice and ``Adam.step()`` as some hundred small launches and six
host waits per minibatch. Here they are six launches (csrc/ppo_update.hpp) and no host wait:

``ppo_loss``                 the loss as one autograd function: two launches forward, one backward;
``device_clip_adam_step``    the gradient norm of every param group, the clip and torch's Adam on the optimiser's OWN state, three
                             launches whatever the number of tensors, so ``optimizer.step()`` and this are interchangeable at any update;
``DevicePPOTrainer``         the reference trainer's constructor, ``ppo_update`` and ``train`` over the two.
"""
import ctypes as C

import numpy as np
import torch

from . import capi
from .policy import UnsupportedPolicy
from .train_common import Launch

_ENTRY = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("numel", "<i8"), ("group", "<i4"), ("first_chunk", "<i4"),
                   ("lr", "<f8"), ("eps", "<f8"), ("beta1", "<f8"), ("beta2", "<f8"), ("bias_correction1", "<f8"), ("bias_correction2", "<f8")])
assert _ENTRY.itemsize == C.sizeof(capi.AcOptimEntry)
STAT_NAMES = ("loss", "policy_loss", "value_loss", "policy_entropy_loss", "ratio")   # the first entries of the stats vector


def constants():
    """The kernels' constants: rows of the loss per workgroup pass, its workgroups at most, elements per optimiser chunk, table entries
    and param groups at most."""
    lib = capi.load_library()
    return {k: lib.ac_ppo_update_constant(i) for i, k in enumerate(("loss_rows", "loss_workgroups", "chunk", "max_entries", "max_groups"))}


class DevicePPOLossFunction(torch.autograd.Function):
    """(values, logp, ent, old_logp, adv, returns, value_preds, active or None, clip, vcoef, ecoef, clipped) -> (loss 0-dim, stats [8]).
    The row arrays are contiguous float32 of M elements on one device, ent of any length. The forward already computes dloss/dlogp and
    dloss/dvalues; the backward multiplies them by the upstream gradient, read on the device."""

    @staticmethod
    def forward(ctx, values, logp, ent, old_logp, adv, returns, value_preds, active, clip, vcoef, ecoef, clipped):
        M, n_ent = logp.numel(), ent.numel()
        run = Launch(logp)
        ws = run.workspace("ac_ppo_loss_workspace_floats", M, n_ent)
        stats, loss, dlogp, dvalues = run.empty(capi.AC_PPO_NSTAT), run.empty(), run.empty(M), run.empty(M)
        run("ac_ppo_loss_forward", M, n_ent, old_logp.numel() // M, logp, old_logp, adv, values, value_preds, returns, active, ent, clip, vcoef,
            ecoef, int(clipped), ws, stats, loss, dlogp, dvalues)
        ctx.shapes, ctx.ecoef = (values.shape, logp.shape, ent.shape), ecoef
        ctx.save_for_backward(dlogp, dvalues)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)
        return loss, stats

    @staticmethod
    def backward(ctx, g_loss, _g_stats):
        none = (None,) * 12
        if g_loss is None:
            return none
        dlogp, dvalues = ctx.saved_tensors
        sv, sl, se = ctx.shapes
        M, n_ent = dlogp.numel(), int(np.prod(se, dtype=np.int64))
        run = Launch(dlogp)
        g_loss = g_loss.to(device=run.dev, dtype=torch.float32).contiguous()
        gv, gl, ge = (run.empty(*s) if ctx.needs_input_grad[i] else None for i, s in enumerate((sv, sl, se)))
        run("ac_ppo_loss_backward", M, n_ent, g_loss, dlogp, dvalues, ctx.ecoef, gl, gv, ge)
        return (gv, gl, ge) + none[3:]


def ppo_loss(values, action_log_probs, dist_entropy, old_action_log_probs, advantages, returns, value_preds, *, clip_param, value_loss_coef,
             entropy_coef, use_clipped_value_loss=True, active_masks=None):
    """The reference's loss (ppo_trainer.py:44-61) on the device: ``(loss, stats)``. ``loss`` is a 0-dim tensor with a grad_fn;
    ``stats`` is a dict of detached 0-dim device tensors: loss, policy_loss, value_loss, policy_entropy_loss and ratio (its mean).
    ``action_log_probs`` is [M, 1]; the other row arrays hold M elements, except that ``old_action_log_probs`` may be [M, C] (the
    MAPPO buffer keeps one column per action column): the new log-probability broadcasts against the columns as in the reference,
    the row's term is their sum and ``ratio`` is the mean over all M C. ``dist_entropy`` has any shape (its plain mean is taken).
    With ``active_masks`` the policy and the value mean become sum(. active) / sum(active). Everything must be float32 on one CUDA
    device (UnsupportedPolicy otherwise); a wrong shape is a ValueError."""
    loss, stats = _loss_and_stats(values, action_log_probs, dist_entropy, old_action_log_probs, advantages, returns, value_preds, clip_param,
                                  value_loss_coef, entropy_coef, use_clipped_value_loss, active_masks)
    return loss, {k: stats[i] for i, k in enumerate(STAT_NAMES)}


def _loss_and_stats(values, action_log_probs, dist_entropy, old_action_log_probs, advantages, returns, value_preds, clip_param, value_loss_coef,
                    entropy_coef, use_clipped_value_loss, active_masks):
    """ppo_loss with the stats as the kernel's vector (capi.AC_PPO_STAT_*)."""
    if not isinstance(action_log_probs, torch.Tensor) or action_log_probs.dim() != 2 or action_log_probs.shape[1] != 1:
        raise ValueError(f"ppo_loss: action_log_probs of shape {tuple(getattr(action_log_probs, 'shape', ()))}, expected [M, 1]")
    M, dev = action_log_probs.shape[0], action_log_probs.device
    named = dict(values=values, action_log_probs=action_log_probs, dist_entropy=dist_entropy, old_action_log_probs=old_action_log_probs,
                 advantages=advantages, returns=returns, value_preds=value_preds)
    if active_masks is not None:
        named["active_masks"] = active_masks
    for k, t in named.items():
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device.type != "cuda" or t.device != dev:
            what = f"{t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise UnsupportedPolicy(f"ppo_loss: {k} is {what} (only float32 on one CUDA device)")
        if k == "old_action_log_probs" and t.dim() == 2 and t.shape[0] == M and 1 <= t.shape[1] <= 64:
            continue   # [M, C]: action_log_probs broadcasts against the columns, as in the reference
        if k != "dist_entropy" and t.numel() != M:
            raise ValueError(f"ppo_loss: {k} of shape {tuple(t.shape)}, expected {M} elements")
    if M < 1 or dist_entropy.numel() < 1:
        raise ValueError("ppo_loss: no rows")
    flat = {k: t.contiguous() for k, t in named.items()}
    return DevicePPOLossFunction.apply(flat["values"], flat["action_log_probs"], flat["dist_entropy"], flat["old_action_log_probs"],
                                              flat["advantages"], flat["returns"], flat["value_preds"], flat.get("active_masks"),
                                              float(clip_param), float(value_loss_coef), float(entropy_coef), bool(use_clipped_value_loss))


def _check_adam(optimizer):
    """The (group index, parameter) pairs that have a gradient; UnsupportedPolicy naming the setting for anything the kernel does not run."""
    if type(optimizer) is not torch.optim.Adam:
        raise UnsupportedPolicy(f"device_clip_adam_step: optimizer is {type(optimizer).__name__} (only torch.optim.Adam)")
    bad, todo, dev = [], [], None
    if len(optimizer.param_groups) > constants()["max_groups"]:
        bad.append(f"{len(optimizer.param_groups)} param groups (at most {constants()['max_groups']})")
    for gi, grp in enumerate(optimizer.param_groups):
        for key in ("amsgrad", "maximize", "capturable", "differentiable"):
            if grp.get(key):
                bad.append(f"param group {gi}: {key}=True")
        if grp.get("weight_decay", 0) != 0:
            bad.append(f"param group {gi}: weight_decay={grp['weight_decay']} (only 0)")
        if isinstance(grp["lr"], torch.Tensor) or any(isinstance(b, torch.Tensor) for b in grp["betas"]):
            bad.append(f"param group {gi}: a tensor lr or betas (only Python numbers)")
        for pi, p in enumerate(grp["params"]):
            if p.grad is None:
                continue
            at = f"param group {gi}, parameter {pi}"
            for what, t in (("parameter", p), ("gradient", p.grad)):
                if t.device.type != "cuda":
                    bad.append(f"{at}: {what} on {t.device} (only a CUDA device)")
                elif dev is not None and t.device != dev:
                    bad.append(f"{at}: {what} on {t.device}, others on {dev} (one device)")
                else:
                    dev = t.device
                if t.is_sparse or t.layout != torch.strided:
                    bad.append(f"{at}: {what} is not dense")
                    continue
                if t.dtype != torch.float32:
                    bad.append(f"{at}: {what} dtype {t.dtype} (only float32)")
                if not t.is_contiguous():
                    bad.append(f"{at}: non-contiguous {what}")
            st = optimizer.state.get(p)
            if st:
                for k in ("exp_avg", "exp_avg_sq"):
                    t = st.get(k)
                    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_contiguous() and t.device == p.device and t.shape == p.shape):
                        bad.append(f"{at}: state {k} is not a contiguous float32 tensor of the parameter's shape and device")
            todo.append((gi, p))
    if len(todo) > constants()["max_entries"]:
        bad.append(f"{len(todo)} parameters with a gradient (at most {constants()['max_entries']})")
    if bad:
        raise UnsupportedPolicy("device_clip_adam_step: " + "; ".join(bad))
    return todo


def device_clip_adam_step(optimizer, max_grad_norm, clip=True):
    """``clip_grad_norm_(group's parameters, max_grad_norm)`` for every param group of a ``torch.optim.Adam`` and then its ``step()``,
    in three launches and without a host wait. Returns the groups' gradient norms before clipping as a device tensor [n_groups]. With
    ``clip=False`` the norms are only reported. ``p.grad`` is left holding the clipped gradient, as the reference leaves it.

    It works on ``optimizer.state`` itself: ``step`` (the CPU tensor torch keeps), ``exp_avg``, ``exp_avg_sq``, created as
    ``torch.optim.Adam`` creates them, so state_dict / load_state_dict and ``optimizer.step()`` keep working in between. A parameter
    without a gradient gets no state and no update. Everything is checked before anything is touched; refused with UnsupportedPolicy
    naming the setting: another optimiser class, amsgrad, weight_decay, maximize, capturable, differentiable, a tensor lr, a
    non-float32, non-contiguous or non-CUDA parameter or gradient."""
    todo = _check_adam(optimizer)
    groups = optimizer.param_groups
    if not todo:
        devs = [p.device for g in groups for p in g["params"]]
        return torch.zeros(len(groups), dtype=torch.float32, device=devs[0] if devs else "cpu")
    run = Launch(todo[0][1])
    host = torch.empty(len(todo) * _ENTRY.itemsize, dtype=torch.uint8, pin_memory=True)
    tab = host.numpy().view(_ENTRY)
    step_dtype = torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32
    for i, (gi, p) in enumerate(todo):
        st, grp = optimizer.state[p], groups[gi]
        if len(st) == 0:   # as torch.optim.Adam._init_group
            st["step"] = torch.tensor(0.0, dtype=step_dtype)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if not torch.is_tensor(st["step"]):
            st["step"] = torch.tensor(float(st["step"]), dtype=step_dtype)
        st["step"] += 1
        step = float(st["step"])
        b1, b2 = (float(b) for b in grp["betas"])
        tab[i] = (p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(), gi, 0,
                  float(grp["lr"]), float(grp["eps"]), b1, b2, 1.0 - b1 ** step, 1.0 - b2 ** step)
    n, ng = len(todo), len(groups)
    ws = run.workspace("ac_optim_workspace_floats", host.data_ptr(), n, ng)   # lays the chunks out in the host table
    # pinned memory, copied on the current stream: torch's host allocator orders the reuse of `host` after the copy
    d_tab = host.to(run.dev, non_blocking=True)
    norms = run.empty(ng)
    run("ac_optim_grad_norms", host, d_tab, n, ng, ws, norms)
    run("ac_optim_clip_adam_step", host, d_tab, n, ng, norms, float(max_grad_norm), int(bool(clip)))
    return norms


class DevicePPOTrainer:
    """The reference's ``PPOTrainer(args, device)`` (PPO and MAPPO) with the update's tail on the device. ``ppo_update(policy, sample)``
    takes the PPO sample (9 entries) or the MAPPO sample (11 entries: the critic reads share_obs), calls ``policy.evaluate_actions`` as
    the reference does, then ``ppo_loss``, ``optimizer.zero_grad()``, ``backward()`` and ``device_clip_adam_step``; between an
    on-device sample and its return nothing waits for the device. It returns the reference's six values as 0-dim device tensors;
    ``ratio`` is its MEAN (the reference returns the [M, 1] tensor, of which ``train`` only takes ``.mean().item()``, which still
    works). ``policy.optimizer`` must have the reference's two param groups, actor then critic.

    The reference's MAPPO trainer does not weight its losses by active_masks; ``args.use_policy_active_masks = True`` (absent: False)
    makes the 11-entry sample's policy and value means sum(. active) / sum(active)."""

    KEYS = ("value_loss", "policy_loss", "policy_entropy_loss", "actor_grad_norm", "critic_grad_norm", "ratio")   # of train_info, in its order
    _ROW = ("policy_loss", "value_loss", "policy_entropy_loss", "ratio", "actor_grad_norm", "critic_grad_norm")   # as ppo_update returns them

    def __init__(self, args, device=torch.device("cpu")):
        self.device = torch.device(device)
        self.tpdv = dict(dtype=torch.float32, device=self.device)
        self.ppo_epoch = args.ppo_epoch
        self.clip_param = args.clip_param
        self.use_clipped_value_loss = args.use_clipped_value_loss
        self.num_mini_batch = args.num_mini_batch
        self.value_loss_coef = args.value_loss_coef
        self.entropy_coef = args.entropy_coef
        self.use_max_grad_norm = args.use_max_grad_norm
        self.max_grad_norm = args.max_grad_norm
        self.use_recurrent_policy = args.use_recurrent_policy
        self.data_chunk_length = args.data_chunk_length
        self.use_policy_active_masks = bool(getattr(args, "use_policy_active_masks", False))
        self.use_stream_ordered_minibatches = bool(getattr(args, "use_stream_ordered_minibatches", False))

    def _to(self, x):
        return (torch.from_numpy(x) if isinstance(x, np.ndarray) else x).to(**self.tpdv)

    def _update(self, policy, sample):
        """(stats vector, group norms) of one update, both on the device."""
        if len(sample) == 9:
            obs, actions, masks, old_logp, adv, returns, vpreds, rnn_a, rnn_c = sample
            active, eval_args = None, (obs, rnn_a, rnn_c, actions, masks)
        elif len(sample) == 11:
            obs, share_obs, actions, masks, active, old_logp, adv, returns, vpreds, rnn_a, rnn_c = sample
            eval_args = (share_obs, obs, rnn_a, rnn_c, actions, masks)
        else:
            raise ValueError(f"ppo_update: a sample of {len(sample)} entries (the PPO sample has 9, the MAPPO sample 11)")
        if len(policy.optimizer.param_groups) != 2:
            raise UnsupportedPolicy(f"ppo_update: policy.optimizer has {len(policy.optimizer.param_groups)} param groups (the reference's two: actor, critic)")
        old_logp, adv, returns, vpreds = self._to(old_logp), self._to(adv), self._to(returns), self._to(vpreds)
        active = self._to(active) if (active is not None and self.use_policy_active_masks) else None
        values, logp, ent = policy.evaluate_actions(*eval_args)
        loss, stats = _loss_and_stats(values, logp, ent.reshape(-1), old_logp, adv, returns, vpreds, self.clip_param, self.value_loss_coef,
                                      self.entropy_coef, self.use_clipped_value_loss, active)
        policy.optimizer.zero_grad()
        loss.backward()
        norms = device_clip_adam_step(policy.optimizer, self.max_grad_norm, clip=self.use_max_grad_norm)
        return stats, norms

    def ppo_update(self, policy, sample):
        stats, norms = self._update(policy, sample)
        return stats[capi.AC_PPO_STAT_POLICY_LOSS], stats[capi.AC_PPO_STAT_VALUE_LOSS], stats[capi.AC_PPO_STAT_ENTROPY_LOSS], \
            stats[capi.AC_PPO_STAT_RATIO_MEAN], norms[0], norms[1]

    @staticmethod
    def _device_list(buffer):
        """The list of two or more device buffers ``buffer`` is, or None (one buffer, or only the reference's host buffers). A list
        that mixes host and device buffers is a ValueError: the two gather in different places."""
        from .rollout_buffer import DeviceReplayBuffer
        if not isinstance(buffer, (list, tuple)) or len(buffer) < 2:
            return None
        on_device = [isinstance(b, DeviceReplayBuffer) for b in buffer]
        if any(on_device) and not all(on_device):
            raise ValueError("train: a list that mixes the reference's host buffers with device buffers (train on one kind: the host "
                             "buffers gather on the host, the device buffers in one launch)")
        return list(buffer) if all(on_device) else None

    def _generator(self, buffer, chunk_order=None):
        from .rollout_buffer import DeviceReplayBuffer, DeviceSharedReplayBuffer
        n, L = self.num_mini_batch, self.data_chunk_length
        several = self._device_list(buffer)
        if several is not None:   # the list form, for both buffer classes
            return DeviceReplayBuffer.recurrent_generator(several, n, L, chunk_order=chunk_order, on_device=True)
        one = buffer[0] if isinstance(buffer, (list, tuple)) and len(buffer) == 1 else buffer
        if isinstance(one, DeviceSharedReplayBuffer):
            return one.recurrent_generator(None, n, L, chunk_order=chunk_order, on_device=True)
        if isinstance(one, DeviceReplayBuffer):
            return DeviceReplayBuffer.recurrent_generator(one, n, L, chunk_order=chunk_order, on_device=True)
        if chunk_order is not None:
            raise ValueError("train: chunk_orders is for the device buffers (the reference's draw their own permutation)")
        if hasattr(one, "share_obs"):   # the reference's SharedReplayBuffer (mappo/ppo_trainer.py:90)
            return buffer.recurrent_generator(buffer.advantages, n, L)
        return type(one).recurrent_generator(buffer, n, L)   # the reference's ReplayBuffer, or a list of them (ppo_trainer.py:87)

    def _epoch(self, buffer, chunk_order=None):
        """One epoch's minibatches of a device buffer from one launch (``buffer.epoch``), no host wait."""
        from .rollout_buffer import DeviceReplayBuffer
        several = self._device_list(buffer)
        if several is not None:   # one launch over the stack of the list's buffers
            return DeviceReplayBuffer.epoch_of(several, self.num_mini_batch, self.data_chunk_length, chunk_order=chunk_order)
        one = buffer[0] if isinstance(buffer, (list, tuple)) and len(buffer) == 1 else buffer
        if not isinstance(one, DeviceReplayBuffer):
            raise ValueError("train: stream_ordered minibatches need a DeviceReplayBuffer / DeviceSharedReplayBuffer (the reference's buffers gather on the host)")
        return one.epoch(self.num_mini_batch, self.data_chunk_length, chunk_order=chunk_order)

    def train(self, policy, buffer, chunk_orders=None, stream_ordered=None):
        """The reference's ``train``: ppo_epoch passes over num_mini_batch minibatches, and the same ``train_info`` dict with the same
        averaging. Every minibatch's six scalars go to one row of a device tensor that is read once at the end. ``buffer`` is one of
        the reference's buffers or a DeviceReplayBuffer / DeviceSharedReplayBuffer (asked for ``on_device=True``). ``chunk_orders``
        (tests): one chunk permutation per epoch for a device buffer instead of torch.randperm. ``buffer`` may also be a list of up to
        8 device buffers of one shape (``DeviceReplayBuffer.recurrent_generator`` / ``epoch_of`` of the list, on either path: one
        permutation over the stack of their sequence views, as the reference's generator treats a list of its buffers); a list that
        mixes host and device buffers is a ValueError.

        ``stream_ordered`` (None: ``args.use_stream_ordered_minibatches``, absent: False): each epoch is one ``buffer.epoch(...)`` on
        torch's current stream instead of the generator, whose every minibatch waits for the device twice; the read at the end is
        then the only host wait of the whole call. Without ``chunk_orders`` the permutations come from torch's DEVICE generator
        (``buffer.epoch``). A device buffer only: ValueError otherwise."""
        if not self.use_recurrent_policy:
            raise NotImplementedError
        if stream_ordered is None:
            stream_ordered = self.use_stream_ordered_minibatches
        num_updates = self.ppo_epoch * self.num_mini_batch
        rows = torch.zeros(num_updates, 6, **self.tpdv)
        i = 0
        for epoch in range(self.ppo_epoch):
            order = None if chunk_orders is None else chunk_orders[epoch]
            for sample in (self._epoch(buffer, order) if stream_ordered else self._generator(buffer, order)):
                stats, norms = self._update(policy, sample)
                rows[i, :4].copy_(stats[capi.AC_PPO_STAT_POLICY_LOSS:capi.AC_PPO_STAT_RATIO_MEAN + 1])   # in the order of _ROW
                rows[i, 4:].copy_(norms)
                i += 1
        host = rows.cpu().double().numpy()   # the one read
        return {k: float(host[:, self._ROW.index(k)].sum() / num_updates) for k in self.KEYS}
