"""Cases, inputs and the tests' own restatements of the reference's ACTLayer.evaluate_actions (algorithms/utils/act.py,
distributions.py) for the training action heads (aircombat-selfplay_amd/act_train.py), shared by
tests/golden/make_act_train_golden.py and the tests.

Every input comes from policy_util.hashed (an exact integer hash), so tests/golden/act_train.npz holds only the reference's outputs
and gradients, as float32 plus one float64 projection per array (``<key>@p``: the dot product with a hashed vector) that the float64
restatement is held to at 1e-12. A case's loss is <action_log_probs, g1> + <dist_entropy, g2> with hashed g1, g2.

Two restatements live here. ``evaluate`` is the formulas in the tests' own words, on a dict of tensors (any dtype, autograd). ``Act``
is a module with the reference's child names (``mlp``, ``action_outs.<i>.logits_net``, ``action_outs.<i>.net``) whose
``evaluate_actions`` and ``forward`` go through torch.distributions head by head as the reference's do: the eager path that
use_device_act replaces, and what the GPU tests time the device against. Below them: the restated actor and policy for a whole
ppo_update (the critic, GRU, MLP and ppo_update are mlp_train_util's)."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import mlp_train_util as MU
from policy_util import hashed

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "act_train.npz")
H = 128
# name -> (M rows, nvec, shoot heads (= shoot columns), active_masks)
CASES = {
    "small": (77, (3, 5, 3), 0, False),                        # M not a multiple of the row tile
    "one": (1, (3, 5, 3, 2), 0, False),                        # a single row; a head of two
    "wide": (40, (41, 41, 41, 30), 0, False),                  # 153 logits; heads straddling the 16-unit slices
    "eight": (33, (2, 37, 16, 31, 19, 23, 3, 29), 0, False),   # eight heads, 160 logits: the limits themselves
    "shoot4": (50, (3, 5, 3), 4, True),                        # last-head rule; every prior value; some rows inactive
    "shoot1": (19, (41, 41, 41, 30), 1, False),                # the other tuple form
    "sharp": (24, (3, 5, 3), 4, False),                        # underflowing probabilities, exact ties, softplus thresholds and saturations
}
SHARP_ZERO_ROWS = (7, 16)           # of case "sharp": x = 0 there, and every head's biases are equal, so its logits tie exactly
ALPHA0, BETA0 = (3.0, 6.0, 10.0), (10.0, 6.0, 3.0)


def spec(case):
    """(M, nvec, shoot heads, active_masks) of a case: its name in CASES, or such a tuple itself (the GPU tests' larger shapes)."""
    return CASES[case] if isinstance(case, str) else case


def n_heads(name):
    _, nvec, ns, _ = spec(name)
    return len(nvec) + ns


def used_heads(name):
    """Indices into action_outs of the heads that take part: the categorical ones and, in a tuple space, only the last."""
    _, nvec, ns, _ = spec(name)
    return list(range(len(nvec))) + ([len(nvec) + ns - 1] if ns else [])


def pnames(name):
    _, nvec, ns, _ = spec(name)
    kinds = ["logits_net"] * len(nvec) + ["net"] * ns
    return [f"action_outs.{i}.{k}.{t}" for i, k in enumerate(kinds) for t in ("weight", "bias")]


def keys(name):
    """The results of a case: no gradient for the shoot heads that take no part."""
    return ("logp", "ent", "dx") + tuple(f"{k}{i}" for i in used_heads(name) for k in ("dW", "db"))


def inputs(name):
    """float32 numpy inputs of a case: the heads' parameters in state_dict naming, x [M, 128], action [M, n_cat + shoot columns],
    g1, g2 [M, 1], and where the case has them alpha0, beta0, active_masks [M, 1]."""
    M, nvec, ns, masked = CASES[name]
    k = 100 * (list(CASES).index(name) + 1)
    sizes = list(nvec) + [2] * ns
    p = {}
    for i, (n, wn) in enumerate(zip(sizes, pnames(name)[0::2])):
        p[wn] = (hashed(k + 2 * i, n * H) * np.float32(0.25)).reshape(n, H)
        p[wn[:-6] + "bias"] = hashed(k + 2 * i + 1, n) * np.float32(0.5)
    x = hashed(k + 40, M * H).reshape(M, H) * np.float32(2.0)
    if name == "sharp":
        for i, n in enumerate(nvec):
            p[f"action_outs.{i}.logits_net.weight"] *= np.float32(40.0)                  # logit gaps beyond 100 ...
            p[f"action_outs.{i}.logits_net.bias"] = np.full(n, 0.25 * (i + 1), np.float32)   # ... and equal biases: ties where x = 0
        x[:, 0] = np.linspace(-2.0, 2.0, M).astype(np.float32)
        x[:, 1] = x[::-1, 0]
        x[list(SHARP_ZERO_ROWS)] = 0.0
        w = np.zeros((2, H), np.float32)
        w[0, 0] = w[1, 1] = 37.5                                                         # y = 45 + 37.5 x: -30 .. 120 down the rows, and back
        last = len(nvec) + ns - 1
        p[f"action_outs.{last}.net.weight"], p[f"action_outs.{last}.net.bias"] = w, np.full(2, 45.0, np.float32)
    u = (hashed(k + 41, M * len(sizes)).reshape(M, len(sizes)).astype(np.float64) + 1.0) / 2.0
    action = np.minimum(np.floor(u * np.array(sizes)), np.array(sizes) - 1).astype(np.float32)
    p.update(x=x, action=action, g1=hashed(k + 42, M).reshape(M, 1), g2=hashed(k + 43, M).reshape(M, 1))
    if ns:
        pick = lambda seed, vals: np.array(vals, np.float32)[np.minimum(((hashed(seed, M).astype(np.float64) + 1.0) * 1.5).astype(int), 2)].reshape(M, 1)
        p.update(alpha0=pick(k + 44, ALPHA0), beta0=pick(k + 45, BETA0))
    if masked:
        p["active_masks"] = (hashed(k + 46, M) > -0.6).astype(np.float32).reshape(M, 1)
    return p


def projector(key, n):
    return hashed(9300 + sum(ord(c) for c in key), n).astype(np.float64)


def project(key, a):
    a = np.asarray(a, np.float64).ravel()
    return float(a @ projector(key, a.size))


def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


# ---- the formulas, in the tests' own words
def _softplus0(t):
    return torch.clamp(t, min=0) + torch.log1p(torch.exp(-torch.abs(t)))   # log(1 + e^t), no threshold


def evaluate(p, x, action, nvec, ns, active_masks=None, alpha0=None, beta0=None):
    """(action_log_probs, dist_entropy), both [M, 1], from a dict of tensors in state_dict naming."""
    M, nc = x.shape[0], len(nvec)
    logp, ent = x.new_zeros(M, 1), x.new_zeros(M, 1)
    for i in range(nc):
        logits = x @ p[f"action_outs.{i}.logits_net.weight"].T + p[f"action_outs.{i}.logits_net.bias"]
        ls = logits - torch.logsumexp(logits, -1, keepdim=True)
        logp = logp + ls.gather(-1, action[:, i:i + 1].long())
        ent = ent - (ls.exp() * ls).sum(-1, keepdim=True)             # an underflowed probability: 0 * finite = 0
    if ns:
        last = nc + ns - 1                                            # only the last shoot head, on every shoot column
        y = x @ p[f"action_outs.{last}.net.weight"].T + p[f"action_outs.{last}.net.bias"]
        u = 100 - F.softplus(100 - F.softplus(y))                     # torch's softplus: identity above 20
        prob = (1 + u[:, :1] + alpha0) / (2 + u[:, :1] + u[:, 1:] + alpha0 + beta0)
        eps = torch.finfo(x.dtype).eps
        pc = prob.clamp(eps, 1 - eps)
        lg = torch.log(pc) - torch.log1p(-pc)
        v = action[:, nc:]
        logp = logp + (v * lg - _softplus0(lg)).sum(-1, keepdim=True)
        ent = ent + (_softplus0(lg) - prob * lg)                      # once, whatever the number of columns
    if active_masks is not None:
        return logp, ent * active_masks / active_masks.sum()
    return logp, ent / M


# ---- the reference's ACTLayer, restated with its child names: the eager path
class CatHead(nn.Module):
    def __init__(self, n, i=H, bias=True):
        super().__init__()
        self.logits_net = nn.Linear(i, n, bias=bias)

    def forward(self, x):
        return torch.distributions.Categorical(logits=self.logits_net(x))


class ShootHead(nn.Module):
    def __init__(self, i=H):
        super().__init__()
        self.net = nn.Linear(i, 2)

    def forward(self, x, **kw):
        u = 100 - F.softplus(100 - F.softplus(self.net(x)))
        a, b = 1 + u[:, 0].unsqueeze(-1), 1 + u[:, 1].unsqueeze(-1)
        return torch.distributions.Bernoulli(probs=(a + kw["alpha0"]) / (a + kw["alpha0"] + b + kw["beta0"]))


class Act(nn.Module):
    """ACTLayer for MultiDiscrete(nvec) (ns = 0) and Tuple(MultiDiscrete(nvec), Discrete(2) | MultiDiscrete([2] * 4)) (ns = 1 | 4)."""

    def __init__(self, nvec, ns=0, mlp=False, in_features=H, bias=True):
        super().__init__()
        self._mlp_actlayer = mlp
        if mlp:
            self.mlp = MU.MLP(H)
        self.action_outs = nn.ModuleList([CatHead(n, in_features, bias) for n in nvec] + [ShootHead(in_features) for _ in range(ns)])
        self._nc, self._ns = len(nvec), ns

    def forward(self, x, deterministic=False, **kw):   # the sampling path (not what use_device_act changes)
        if self._mlp_actlayer:
            x = self.mlp(x)
        acts, lps = [], []
        for h in self.action_outs[:self._nc]:
            d = h(x)
            a = d.probs.argmax(-1, keepdim=True) if deterministic else d.sample().unsqueeze(-1)
            acts.append(a.float())
            lps.append(d.log_prob(a.squeeze(-1)).unsqueeze(-1))
        for h in self.action_outs[self._nc:]:
            d = h(x, **kw)
            acts.append((d.probs > 0.5).float() if deterministic else d.sample())
        return torch.cat(acts, -1), torch.cat(lps, -1).sum(-1, keepdim=True)

    def evaluate_actions(self, x, action, active_masks=None, **kw):
        if self._mlp_actlayer:
            x = self.mlp(x)
        scale = (lambda e: e * active_masks / active_masks.sum()) if active_masks is not None else (lambda e: e / x.shape[0])
        lps, ents = [], []
        for i, h in enumerate(self.action_outs[:self._nc]):
            d = h(x)
            lps.append(d.log_prob(action[:, i]).unsqueeze(-1))
            ents.append(scale(d.entropy().unsqueeze(-1)))
        if self._ns:
            d = self.action_outs[-1](x, **kw)
            lps.append(d.log_prob(action[:, self._nc:]).sum(-1, keepdim=True))
            ents.append(scale(d.entropy().sum(-1, keepdim=True)))
        return torch.cat(lps, -1).sum(-1, keepdim=True), torch.cat(ents, -1).sum(-1, keepdim=True)


def act_from(name, inp, device="cpu", dtype=torch.float32):
    _, nvec, ns, _ = spec(name)
    m = Act(nvec, ns)
    m.load_state_dict({k: torch.as_tensor(inp[k]) for k in pnames(name)})
    return m.to(device=device, dtype=dtype)


def run_with_grads(eval_fn, params, x, inp, name):
    """Forward + backward of <logp, g1> + <ent, g2>; ``eval_fn(x, action, active_masks, **prior) -> (logp, ent)``, ``params`` the
    heads' parameter tensors (leaf, requires_grad) as a dict in state_dict naming. Returns keys(name) as float64 numpy arrays and the
    indices of the heads whose weight got no gradient."""
    t = lambda k: torch.as_tensor(inp[k]).to(device=x.device, dtype=x.dtype) if k in inp else None
    prior = {"alpha0": t("alpha0"), "beta0": t("beta0")} if "alpha0" in inp else {}
    logp, ent = eval_fn(x, t("action"), t("active_masks"), **prior)
    ((logp * t("g1")).sum() + (ent * t("g2")).sum()).backward()
    np64 = lambda v: v.detach().double().cpu().numpy()
    out = {"logp": np64(logp), "ent": np64(ent), "dx": np64(x.grad)}
    names = pnames(name)
    for i in used_heads(name):
        out[f"dW{i}"], out[f"db{i}"] = np64(params[names[2 * i]].grad), np64(params[names[2 * i + 1]].grad)
    unused = [i for i in range(n_heads(name)) if params[names[2 * i]].grad is None and params[names[2 * i + 1]].grad is None]
    return out, unused


# ---- the restated actor and policy for a whole ppo_update (mlp_train_util's, with the heads as an Act module that is called)
class Actor(nn.Module):
    def __init__(self, obs=MU.OBS, nvec=MU.NVEC, ns=0, **kw):
        super().__init__()
        self.base, self.rnn = MU.Base(obs), MU.RefGRULayer()
        self.act = Act(nvec, ns, mlp=True, **kw)

    def evaluate_actions(self, obs, rnn_states, action, masks, active_masks=None, **prior):
        x, _ = self.rnn(self.base(obs), rnn_states, masks)
        return self.act.evaluate_actions(x, action, active_masks, **prior)


class Policy(MU.Policy):
    def __init__(self, seed, device="cuda", critic_obs=MU.OBS, **kw):
        torch.manual_seed(seed)
        self.actor, self.critic = Actor(**kw).to(device), MU.Critic(critic_obs).to(device)
        self.optimizer = torch.optim.Adam([{"params": self.actor.parameters()}, {"params": self.critic.parameters()}], lr=5e-4, eps=1e-5)
