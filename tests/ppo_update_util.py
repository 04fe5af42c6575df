"""Inputs and the tests' own float64 restatements for the update's tail on the device (aircombat-selfplay_amd/ppo_update.py): the
reference's loss (algorithms/ppo/ppo_trainer.py:44-61), torch's clip_grad_norm_ and torch's single-tensor Adam. Shared by
tests/golden/make_ppo_update_golden.py and the tests. Every input comes from policy_util.hashed, so tests/golden/ppo_update.npz holds
only what the reference's own PPOTrainer.ppo_update returned and left in its policy and optimiser.

The golden's policy is a stub: its ``evaluate_actions`` is a small differentiable function of two parameter sets (a 12-input Linear
each), scaled so that the actor's gradient norm stays below max_grad_norm = 2 and the critic's far above it."""
import os
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from policy_util import hashed

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_update.npz")
ARGS = dict(ppo_epoch=2, clip_param=0.2, use_clipped_value_loss=True, num_mini_batch=2, value_loss_coef=1.0, entropy_coef=0.01,
            use_max_grad_norm=True, max_grad_norm=2.0, use_recurrent_policy=True, data_chunk_length=8)
LR, ADAM_EPS, BETAS = 5e-4, 1e-5, (0.9, 0.999)
STUB_OBS, STUB_M, STUB_STEPS, VALUE_SCALE = 12, 40, 3, 30.0
RETURNED = ("policy_loss", "value_loss", "policy_entropy_loss", "ratio", "actor_grad_norm", "critic_grad_norm")
PNAMES = ("actor.weight", "actor.bias", "critic.weight", "critic.bias")


def trainer_args(**over):
    return types.SimpleNamespace(**{**ARGS, **over})


# ---- the loss
def loss_inputs(M, n_ent, seed=1, old_cols=1):
    """float32 numpy inputs of the loss, M rows: ratios on both sides of 1 +- 0.2, values on both sides of value_preds +- 0.2, and
    rows with adv = 0 (i % 7 == 3), logp == old_logp (i % 11 == 5), values == value_preds (i % 13 == 6); active_masks with zeros. With
    ``old_cols`` > 1 old_action_log_probs is [M, old_cols] as the MAPPO buffer keeps it, the further columns within +-0.3 of the first."""
    h = lambda k, n: hashed(seed * 100 + k, n)
    i = np.arange(M)
    old = np.float32(-2.0) + np.float32(0.5) * h(1, M)
    logp = old + np.float32(0.5) * h(2, M)
    adv = np.float32(2.0) * h(3, M)
    vp = np.float32(3.0) * h(4, M)
    v = vp + np.float32(0.6) * h(5, M)
    R = vp + h(6, M)
    adv[i % 7 == 3] = 0.0
    logp[i % 11 == 5] = old[i % 11 == 5]
    v[i % 13 == 6] = vp[i % 13 == 6]
    active = (h(7, M) > np.float32(-0.7)).astype(np.float32)
    active[0] = 1.0
    col = lambda a: np.ascontiguousarray(a.reshape(M, 1))
    olds = np.concatenate([col(old)] + [col(old + np.float32(0.3) * h(10 + c, M)) for c in range(1, old_cols)], axis=1)
    return dict(values=col(v), action_log_probs=col(logp), dist_entropy=(np.float32(1.0) + np.float32(0.5) * h(8, n_ent)).reshape(n_ent, 1),
                old_action_log_probs=olds, advantages=col(adv), returns=col(R), value_preds=col(vp), active_masks=col(active))


def loss_torch(t, clip=0.2, vcoef=1.0, ecoef=0.01, clipped=True, use_active=False):
    """The reference's lines 44-61 on a dict of tensors of any dtype (autograd decides the gradient conventions); with ``use_active``
    the two means as tests/mlp_train_util.ppo_update states them. Returns the five stats as 0-dim tensors, loss first."""
    values, logp, ent = t["values"], t["action_log_probs"], t["dist_entropy"]
    old, adv, returns, vpreds = t["old_action_log_probs"], t["advantages"], t["returns"], t["value_preds"]
    ratio = torch.exp(logp - old)
    surr1 = ratio * adv
    surr2 = torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv
    pl = torch.sum(torch.min(surr1, surr2), dim=-1, keepdim=True)
    if clipped:
        vpc = vpreds + (values - vpreds).clamp(-clip, clip)
        vl = 0.5 * torch.max((values - returns).pow(2), (vpc - returns).pow(2))
    else:
        vl = 0.5 * (returns - values).pow(2)
    if use_active:
        a = t["active_masks"]
        policy_loss, value_loss = -(pl * a).sum() / a.sum(), (vl * a).sum() / a.sum()
    else:
        policy_loss, value_loss = -pl.mean(), vl.mean()
    pel = -ent.mean()
    return dict(loss=policy_loss + value_loss * vcoef + pel * ecoef, policy_loss=policy_loss, value_loss=value_loss, policy_entropy_loss=pel,
                ratio=ratio.mean())


def loss_with_grads(fn, inp, device, dtype, use_active, upstream=3.0, **kw):
    """Stats and the gradients of ``upstream * loss`` with respect to values, action_log_probs and dist_entropy, as float64 numpy.
    ``fn(tensors, use_active=..., **kw) -> dict of stats`` (loss_torch, or the device's ppo_loss behind an adapter)."""
    t = {k: torch.as_tensor(v).to(device, dtype) for k, v in inp.items()}
    for k in ("values", "action_log_probs", "dist_entropy"):
        t[k].requires_grad_(True)
    stats = fn(t, use_active=use_active, **kw)
    (upstream * stats["loss"]).backward()
    out = {k: stats[k].detach().double().cpu().numpy() for k in ("loss", "policy_loss", "value_loss", "policy_entropy_loss", "ratio")}
    out.update({"d_" + k: t[k].grad.double().cpu().numpy() for k in ("values", "action_log_probs", "dist_entropy")})
    return out


# ---- the clip and Adam, float64 numpy
def clip_coef(norm, max_norm):
    """clip_grad_norm_'s coefficient: clamp(max_norm / (norm + 1e-6), max=1); NaN stays NaN."""
    c = max_norm / (norm + 1e-6)
    return c if (c != c or c < 1.0) else 1.0


def group_norm(grads):
    return float(np.sqrt(sum(float((np.asarray(g, np.float64) ** 2).sum()) for g in grads)))


def adam_f64(p, g, m, v, step, lr=LR, betas=BETAS, eps=ADAM_EPS):
    """torch's single-tensor Adam (no amsgrad, no weight decay) on float64 arrays: (p, m, v) after step number ``step``."""
    b1, b2 = betas
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    p = p - (lr / (1.0 - b1 ** step)) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + eps)
    return p, m, v


def clip_adam_f64(groups, state, max_norm, clip=True, **adam):
    """``groups``: a list of lists of (key, p, g) float64 arrays, g None for a parameter without a gradient. ``state``: key -> dict(step,
    m, v), updated in place. Returns (norms, {key: new p}, {key: clipped g})."""
    norms, new_p, new_g = [], {}, {}
    for grp in groups:
        norm = group_norm([g for _, _, g in grp if g is not None])
        norms.append(norm)
        coef = clip_coef(norm, max_norm) if clip else 1.0
        for key, p, g in grp:
            if g is None:
                continue
            st = state.setdefault(key, dict(step=0, m=np.zeros_like(p), v=np.zeros_like(p)))
            st["step"] += 1
            with np.errstate(invalid="ignore"):
                g = g * coef
                new_p[key], st["m"], st["v"] = adam_f64(p, g, st["m"], st["v"], st["step"], **adam)
            new_g[key] = g
    return norms, new_p, new_g


# ---- the golden's stub policy and its samples
class StubPolicy:
    """What the reference's ppo_update needs of a policy: actor and critic are one Linear(12, 1) each, ``evaluate_actions`` accepts the
    PPO (5) and the MAPPO (6, cent_obs first) argument lists, ``optimizer`` is a real Adam over {actor}, {critic}."""

    def __init__(self, dtype=torch.float64, device="cpu"):
        self.actor, self.critic = nn.Linear(STUB_OBS, 1), nn.Linear(STUB_OBS, 1)
        with torch.no_grad():
            self.actor.weight.copy_(torch.as_tensor(hashed(701, STUB_OBS) * np.float32(0.3)).view(1, -1))
            self.actor.bias.copy_(torch.as_tensor(hashed(702, 1) * np.float32(0.1)))
            self.critic.weight.copy_(torch.as_tensor(hashed(703, STUB_OBS) * np.float32(0.5)).view(1, -1))
            self.critic.bias.copy_(torch.as_tensor(hashed(704, 1) * np.float32(0.1)))
        self.actor.to(device, dtype)
        self.critic.to(device, dtype)
        self.optimizer = torch.optim.Adam([{"params": self.actor.parameters()}, {"params": self.critic.parameters()}], lr=LR, eps=ADAM_EPS)

    def params(self):
        return dict(zip(PNAMES, (self.actor.weight, self.actor.bias, self.critic.weight, self.critic.bias)))

    def evaluate_actions(self, *a):
        cent, obs = (a[0], a[1]) if len(a) == 6 else (a[0], a[0])
        as_t = lambda x: torch.as_tensor(x).to(self.actor.weight)
        z = self.actor(as_t(obs))
        logp = -F.softplus(z) - 1.5
        ent = 0.5 * F.softplus(-z)
        return VALUE_SCALE * self.critic(as_t(cent)), logp, ent


def stub_sample(step, mappo):
    """The float32 numpy sample of update ``step`` (0 ..), in the reference's order: 9 entries, or 11 for MAPPO."""
    M, h = STUB_M, lambda k, n: hashed(800 + 20 * step + k, n)
    col = lambda a: np.ascontiguousarray(a.reshape(M, -1))
    obs, share = col(h(1, M * STUB_OBS)), col(h(2, M * STUB_OBS))
    actions, masks, active = col(np.zeros(M, np.float32)), col(np.ones(M, np.float32)), col((h(3, M) > np.float32(-0.8)).astype(np.float32))
    old = col(np.float32(-2.2) + np.float32(0.3) * h(4, M))
    adv, returns, vp = col(np.float32(1.5) * h(5, M)), col(np.float32(10.0) * h(6, M)), col(np.float32(10.0) * h(7, M))
    vp[::5] += np.float32(0.1) * h(8, M).reshape(M, 1)[::5]
    rnn = np.zeros((M // 8, 1, 128), np.float32)
    if mappo:
        return (obs, share, actions, masks, active, old, adv, returns, vp, rnn, rnn)
    return (obs, actions, masks, old, adv, returns, vp, rnn, rnn)


def restated_update(policy, state, sample, clip=0.2, vcoef=1.0, ecoef=0.01, max_norm=2.0):
    """One update of a float64 StubPolicy by the restatements alone (loss_torch for the loss and, through autograd, its gradient;
    clip_adam_f64 for the rest). ``state``: the Adam state of clip_adam_f64. Returns the reference's six values as floats."""
    old, adv, returns, vp = (torch.as_tensor(x).double() for x in sample[-6:-2])
    eval_args = (sample[0], sample[-2], sample[-1], sample[1], sample[2]) if len(sample) == 9 else \
        (sample[1], sample[0], sample[-2], sample[-1], sample[2], sample[3])
    values, logp, ent = policy.evaluate_actions(*eval_args)
    st = loss_torch(dict(values=values, action_log_probs=logp, dist_entropy=ent, old_action_log_probs=old, advantages=adv, returns=returns,
                         value_preds=vp), clip, vcoef, ecoef)
    ps = policy.params()
    grads = torch.autograd.grad(st["loss"], list(ps.values()))
    np64 = lambda t: t.detach().double().cpu().numpy()
    groups = [[(k, np64(ps[k]), np64(g)) for k, g in list(zip(ps, grads))[:2]], [(k, np64(ps[k]), np64(g)) for k, g in list(zip(ps, grads))[2:]]]
    norms, new_p, _ = clip_adam_f64(groups, state, max_norm)
    with torch.no_grad():
        for k, v in new_p.items():
            ps[k].copy_(torch.as_tensor(v))
    return dict(zip(RETURNED, [float(st[k].detach()) for k in RETURNED[:4]] + norms))


def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}
