"""The rollout policy kernels at the edges of the configurations they accept: one table of configurations, their hashed weights and
inputs, the float64 restatement (policy_util, pinned to the reference by tests/golden/policy_edges.npz), the comparison the GPU test
applies to the device's outputs, and a second restatement that carries one planted fault at a time, which the host test feeds to the
same comparison to show that it can fail (test_policy_edges_host.py, test_gpu_policy_edges.py)."""
import collections
import functools
import os

import numpy as np
import torch

import policy_util as U

N = 250          # rows per entry: seven full 32-row tiles and a ragged one of 26
MARGIN = 1e-4    # a head whose top-two logits (or |p - 0.5|) are this close may take either action
EDGE = 1e-5      # a stochastic row is excused when a uniform lies this close to a CDF edge
GOLDEN = os.path.join(U.GOLDEN_DIR, "policy_edges.npz")
GOLDEN_ROWS = 32

Entry = collections.namedtuple("Entry", "name form obs_dim cent nvec n_shoot fn scale seed derived")


def _entry(name, form, obs_dim, cent, nvec, n_shoot, fn, seed, scale=None, derived=None):
    return Entry(name, form, obs_dim, cent, list(nvec), n_shoot, fn, list(scale or [1.0] * (len(nvec) + n_shoot)), seed, derived)


_BASE = [
    # the PPO form (DevicePolicy): layer 1 padded to K = 32
    _entry("ppo_d1_n2", "ppo", 1, None, [2], 0, True, 301),                     # feature norm of one column: variance 0
    _entry("ppo_d1_n160", "ppo", 1, None, [160], 0, False, 302),
    _entry("ppo_d8_ones", "ppo", 8, None, [1] * 8, 0, True, 303),               # eight size-1 heads
    _entry("ppo_d14_shoot", "ppo", 14, None, [3, 5, 3], 4, False, 304),         # the smallest width the munition prior allows
    _entry("ppo_d16_edges", "ppo", 16, None, [16, 16, 1, 127], 0, False, 305),  # heads on tile edges, a size-1 head between, 160 logits
    _entry("ppo_d31_straddle", "ppo", 31, None, [15, 17, 16, 16, 32, 31, 33], 0, True, 306),   # heads across tile edges, 160 logits
    _entry("ppo_d32_8x20_shoot", "ppo", 32, None, [20] * 8, 4, True, 307),      # 8 + 4 heads, all 176 columns live, no padding column
    _entry("ppo_d32_n160_shoot", "ppo", 32, None, [160], 4, False, 308),
    # the wide form (DeviceMAPPOPolicy): actor width / critic width, 128-column K-blocks of up to four 32-column steps
    _entry("wide_33_32", "mappo", 33, 32, [3, 5, 3], 4, True, 309),
    _entry("wide_128_129", "mappo", 128, 129, [41, 41, 41, 30], 0, True, 310),
    _entry("wide_129_256", "mappo", 129, 256, [20] * 8, 4, False, 311),
    _entry("wide_257_1", "mappo", 257, 1, [7, 9], 0, True, 312),
    _entry("wide_640_640", "mappo", 640, 640, [160], 4, True, 313),
    _entry("wide_639_640", "mappo", 639, 640, [7, 9], 0, True, 314),
]
TIE_ROWS, TIE_FROM, ZERO_HEAD = (3, 11), 7, 1     # ties: head 0's logit rows 3 and 11 copy row 7; head 1 is all zero
SHARP_HEAD, SHARP_LOGIT, SHARP_SHOOT = 2, 40.0, 60.0


def _derive(b):
    sharp = [1.0] * len(b.nvec) + [SHARP_SHOOT] * b.n_shoot
    sharp[SHARP_HEAD] = SHARP_LOGIT
    return [b._replace(name=b.name + "_ties", derived="ties"), b._replace(name=b.name + "_sharp", derived="sharp", scale=sharp)]


ENTRIES = {e.name: e for e in _BASE + [d for b in _BASE if b.name in ("ppo_d32_8x20_shoot", "wide_129_256") for d in _derive(b)]}
NAMES = list(ENTRIES)


def critic_dim(e):
    return e.cent if e.form == "mappo" else e.obs_dim


def state_dicts(e):
    """(actor, critic) state_dicts of an entry: policy_util's seeded recipe plus the munition heads; the critic of the wide form is the
    same recipe on cent_obs_dim. The derived entries plant their ties / scales in the heads."""
    a, c = U.seeded_state_dicts(e.obs_dim, e.nvec, e.fn, seed=e.seed)
    U.add_munition_heads(a, len(e.nvec), e.n_shoot, e.seed)
    if e.form == "mappo":
        c = U.seeded_state_dicts(e.cent, e.nvec, e.fn, seed=e.seed)[1]
    if e.derived == "ties":
        for k in ("weight", "bias"):
            w = a[f"act.action_outs.0.logits_net.{k}"] = a[f"act.action_outs.0.logits_net.{k}"].copy()
            w[list(TIE_ROWS)] = w[TIE_FROM]
            a[f"act.action_outs.{ZERO_HEAD}.logits_net.{k}"] = np.zeros_like(a[f"act.action_outs.{ZERO_HEAD}.logits_net.{k}"])
    if e.derived == "sharp":
        for k in ("weight", "bias"):
            a[f"act.action_outs.{SHARP_HEAD}.logits_net.{k}"] = a[f"act.action_outs.{SHARP_HEAD}.logits_net.{k}"] * np.float32(SHARP_LOGIT)
            for s in range(e.n_shoot):
                a[f"act.action_outs.{len(e.nvec) + s}.net.{k}"] = a[f"act.action_outs.{len(e.nvec) + s}.net.{k}"] * np.float32(SHARP_SHOOT)
    return a, c


def one_head(sd, nvec, head):
    """The actor with head ``head`` cut to size 1 (its first logit row), and that nvec."""
    sd = dict(sd)
    for k in ("weight", "bias"):
        sd[f"act.action_outs.{head}.logits_net.{k}"] = sd[f"act.action_outs.{head}.logits_net.{k}"][:1]
    return sd, [1 if h == head else n for h, n in enumerate(nvec)]


THRESHOLDS = ((11, np.deg2rad(22.5)), (11, np.deg2rad(45.0)), (13, 0.8), (13, 1.2))   # the prior's: 22.5 / 45 degrees, 8000 / 12000 m


def special_rows(e):
    """(all-zero row, row constant at 4.0) of an entry with feature normalisation, else None."""
    return (N - 2, N - 1) if e.fn else None


@functools.lru_cache(maxsize=None)
def inputs(name):
    """obs uniform on +-2 [N, obs_dim], cent_obs (wide form) [N, cent], GRU states, masks (0 on about 20 % of the rows), all from the
    hash. Munition entries: columns 11 / 13 non-negative, rows 0..7 0.5 % on either side of each prior threshold. Feature-norm
    entries: the last two rows are all zero and constant 4.0, with one GRU state and mask between them."""
    e = ENTRIES[name]
    k = e.seed * 1000
    d = {"obs": (np.float32(2.0) * U.hashed(k + 900, N * e.obs_dim)).reshape(N, e.obs_dim),
         "rnn_states": U.hashed_states(k + 901, N), "rnn_states_critic": U.hashed_states(k + 902, N),
         "masks": (U.hashed(k + 903, N) > -0.6).astype(np.float32).reshape(N, 1)}
    if e.form == "mappo":
        d["cent_obs"] = (np.float32(2.0) * U.hashed(k + 904, N * e.cent)).reshape(N, e.cent)
    if e.n_shoot:
        d["obs"][:, 11], d["obs"][:, 13] = np.abs(d["obs"][:, 11]), np.abs(d["obs"][:, 13])
        for col, th in THRESHOLDS:   # no hashed row within 0.5 % of a threshold: float32 and float64 may disagree only at one
            near = np.abs(d["obs"][:, col].astype(np.float64) / th - 1.0) < 5e-3
            d["obs"][near, col] = np.float32(th * 1.01)
        for i, (col, th) in enumerate(THRESHOLDS):
            d["obs"][2 * i, col] = np.float32(th * 0.995)
            d["obs"][2 * i + 1, col] = np.float32(th * 1.005)
    if e.fn:
        z, c = special_rows(e)
        for key in ("obs", "cent_obs"):
            if key in d:
                d[key][z], d[key][c] = 0.0, 4.0
        for key in ("rnn_states", "rnn_states_critic"):
            d[key][c] = d[key][z]
        d["masks"][z] = d["masks"][c] = 1.0
    for v in d.values():
        v.setflags(write=False)
    d["sd"], d["critic_sd"] = state_dicts(e)
    return d


def critic_input(e, d):
    return d["cent_obs"] if e.form == "mappo" else d["obs"]


@functools.lru_cache(maxsize=None)
def reference(name, dtype=torch.float64):
    """policy_util's restatement of an entry (actor and critic outputs in one dict), computed once and shared; float32 gives the eager twin."""
    e, d = ENTRIES[name], inputs(name)
    with U.precision(dtype):
        out = U.actor(d["sd"], d["obs"], d["rnn_states"], d["masks"], e.nvec, e.n_shoot, e.fn)
        out.update(U.critic(d["critic_sd"], critic_input(e, d), d["rnn_states_critic"], d["masks"], e.fn))
    out = {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def prior_f32(obs):
    """alpha0 / beta0 as the device computes them, in float32."""
    ang, dist = obs[:, 11] * np.float32(57.29577951308232), obs[:, 13] * np.float32(10000.0)
    a0 = np.where(dist <= np.float32(8000.0), 10.0, np.where(dist <= np.float32(12000.0), 6.0, 3.0))
    b0 = np.where(ang <= np.float32(22.5), 3.0, np.where(ang <= np.float32(45.0), 6.0, 10.0))
    return a0, b0


# ---- bounds
def logp_factor(e):
    """A head's rounding error enters the summed log-prob once and grows with its logit scale; the bounds were set with 4 to 7 heads."""
    return max(1.0, sum(e.scale) / 4.0)


# (entry, precision, key) -> bound widened on the float32 eager twin's evidence (4 x the twin's own error); none needed
WIDENED = {}


# the zero head's log-prob by difference of two float32 sums of 12 terms: the issue's 2 ulp (of the summed log-prob) is a quarter of
# nothing the float32 twin can do itself -- twin_zero_head_ulps() measures 2.5 and 2.0 ulp -- so the bound is 4 x 2.5
ZERO_HEAD_ULP = 10.0


def twin_zero_head_ulps(name):
    """What float32 itself makes of the zero head's log-prob by difference: each head's log-prob from the restatement's logits in
    float32, summed in head order as the kernel sums them, with and without the zero head; in ulps of the sums."""
    e, r = ENTRIES[name], reference(name)
    lg, n = r["logits"].astype(np.float32), N
    lps = []
    for sl in head_slices(e):
        x = lg[:, sl]
        s = np.zeros(n, np.float32)
        for j in range(x.shape[1]):
            s = s + np.exp(x[:, j] - x.max(-1)).astype(np.float32)
        lps.append(-np.log(s).astype(np.float32))
    for k in range(e.n_shoot):
        p = r["shoot_p"][:, k].astype(np.float32)
        lps.append(np.where(p > 0.5, np.log(p), np.log1p(-p)).astype(np.float32))
    full, one = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for h, l in enumerate(lps):
        full, one = full + l, one + (np.float32(0.0) if h == ZERO_HEAD else l)
    ulp = np.spacing(np.maximum(np.abs(full), np.abs(one))).astype(np.float64)
    return (np.abs((full.astype(np.float64) - one) + np.log(20.0)) / ulp).max()


def bounds(e, precision, tol):
    """{"logp", "h", "v", "slogp"} for an entry: ``tol`` is the form's TOL table (test_gpu_policy.TOL / test_gpu_mappo_policy.TOL)."""
    b = dict(tol[precision])
    b["logp"] = b["logp"] * logp_factor(e)
    b["slogp"] = 1e-4 * logp_factor(e)
    b["zero_head_ulp"] = ZERO_HEAD_ULP
    for k in ("logp", "h", "v"):
        b[k] = WIDENED.get((e.name, precision, k), b[k])
    return b


def twin_errors(name):
    """The float32 eager restatement's own errors against the float64 one: {"logp", "h", "v"}."""
    r, t = reference(name), reference(name, torch.float32)
    same = (r["actions"] == t["actions"]).all(-1)
    return {"logp": np.abs(r["log_probs"] - t["log_probs"])[same].max(),
            "h": max(np.abs(r["rnn_states_out"] - t["rnn_states_out"]).max(), np.abs(r["rnn_states_critic_out"] - t["rnn_states_critic_out"]).max()),
            "v": np.abs(r["values"] - t["values"]).max()}


# ---- the comparison
def head_slices(e):
    off = np.concatenate([[0], np.cumsum(e.nvec)])
    return [slice(int(off[h]), int(off[h + 1])) for h in range(len(e.nvec))]


def planted_heads(e):
    """The heads an entry plants an edge in, which the cap on natural ties does not count: the duplicated and the zero head of
    ``ties``; the munition heads of ``sharp``, whose x 60 saturates both Beta parameters at once, so that p is 0.5 to rounding
    wherever alpha0 equals beta0."""
    if e.derived == "ties":
        return [0, ZERO_HEAD]
    return list(range(len(e.nvec), len(e.nvec) + e.n_shoot)) if e.derived == "sharp" else []


def ambiguous(e, ref):
    """[N, heads] True where the restatement's action is within MARGIN of a tie. The planted heads of a ``ties`` entry are never
    excused for their planted ties: head 0's duplicates are left out of its gap, head 1 has one right answer."""
    cols = []
    for h, sl in enumerate(head_slices(e)):
        lg = ref["logits"][:, sl]
        if e.derived == "ties" and h == 0:
            lg = np.delete(lg, TIE_ROWS, axis=-1)
        if lg.shape[-1] < 2 or (e.derived == "ties" and h == ZERO_HEAD):
            cols.append(np.zeros(len(lg), bool))
            continue
        s = np.sort(lg, -1)
        cols.append(s[:, -1] - s[:, -2] < MARGIN)
    for k in range(e.n_shoot):
        cols.append(np.abs(ref["shoot_p"][:, k] - 0.5) < MARGIN)
    return np.stack(cols, -1)


def zero_head_pick(u):
    """The sampler's pick on 20 equal logits, exactly: e = 1, s = 20 and the running sum j + 1 are exact in float32, so the pick is
    the first j with j + 1 > fl32(u * 20), or the last category when there is none."""
    t = np.asarray(u, np.float32) * np.float32(20.0)
    c = np.arange(1, 21, dtype=np.float32)
    hit = c[None, :] > t[:, None]
    return np.where(hit.any(-1), hit.argmax(-1), 19)


def compare(dev, ref, e, b):
    """Hold a device's outputs of an entry to the restatement's. ``dev``: "v", "a", "lp", "ha", "hc" of the deterministic call (float64
    arrays), optionally "lp_one" (the same call with the zero head cut to size 1) and "stoch", a list of {"u" [N, heads] the call's
    uniforms, "a", "lp"}. ``b``: bounds(). Returns (problems, used): every violated condition in words, and the largest fraction of
    each bound used."""
    bad, used = [], {}
    n_cat = len(e.nvec)
    amb = ambiguous(e, ref)
    a = dev["a"]
    ok = (a == ref["actions"]) | amb
    if not ok.all():
        bad.append(f"{int((~ok).sum())} deterministic actions differ outside tie margins (heads {sorted(set(np.nonzero(~ok)[1]))})")
    exact = (a == ref["actions"]).all(-1)
    if e.derived == "ties" and np.isin(a[:, 0], (TIE_FROM,) + TIE_ROWS[1:]).any():
        bad.append("ties: head 0 took a later copy of a tied maximum (first maximum wanted)")
    ones = [h for h, k in enumerate(e.nvec) if k == 1]
    for h in ones:
        if (a[:, h] != 0).any():
            bad.append(f"size-1 head {h} took a nonzero action")
    if len(ones) == n_cat and not e.n_shoot and (dev["lp"] != 0.0).any():
        bad.append("only size-1 heads, but the log-prob is not exactly 0")

    def hold(key, err, bound):
        used[key] = max(used.get(key, 0.0), float(err) / bound)
        if not err < bound:
            bad.append(f"{key}: {err:.3g} is not below {bound:.3g}")

    if exact.any():
        hold("logp", np.abs(dev["lp"] - ref["log_probs"])[exact].max(), b["logp"])
    hold("h", np.abs(dev["ha"] - ref["rnn_states_out"]).max(), b["h"])
    if dev.get("v") is not None:
        hold("v", np.abs(dev["v"] - ref["values"]).max(), b["v"])
        hold("h", np.abs(dev["hc"] - ref["rnn_states_critic_out"]).max(), b["h"])
    if e.fn:   # the all-zero row and the row constant at 4.0 both reach layer 1 as the feature norm's bias
        z, c = special_rows(e)
        keys = ["ha"] + (["v", "hc"] if dev.get("v") is not None else []) + ([] if e.n_shoot else ["lp"])
        for k in keys:
            if not np.array_equal(dev[k][z], dev[k][c]):
                bad.append(f"the all-zero row and the constant row differ in {k}")
        if not np.array_equal(a[z, :n_cat], a[c, :n_cat]):
            bad.append("the all-zero row and the constant row differ in their categorical actions")
    if dev.get("lp_one") is not None:   # the zero head's own log-prob, by difference: -log 20
        both = exact & (dev["a_one"] == np.where(np.arange(a.shape[1]) == ZERO_HEAD, 0, ref["actions"])).all(-1)
        ulp = np.spacing(np.maximum(np.abs(dev["lp"]), np.abs(dev["lp_one"])).astype(np.float32)).astype(np.float64)
        err = (np.abs((dev["lp"] - dev["lp_one"]) + np.log(20.0)) / ulp)[both].max()
        hold("zero_head_logp", err, b["zero_head_ulp"])
    # ---- the stochastic calls
    excused = np.zeros(len(a), bool)
    for call in dev.get("stoch", ()):
        u, sa = call["u"].astype(np.float64), call["a"]
        want = np.zeros(len(a))
        for h, sl in enumerate(head_slices(e)):
            pr = ref["probs"][:, sl]
            pick, edge = U.inverse_cdf(pr, u[:, h])
            if e.derived == "ties" and h == ZERO_HEAD:   # exact, no excusals
                pick = zero_head_pick(call["u"][:, h])
                if not (sa[:, h] == pick).all():
                    bad.append(f"ties: {int((sa[:, h] != pick).sum())} picks of the zero head are not the first j with j + 1 > fl32(20 u)")
            else:
                excused |= edge < EDGE
                miss = (sa[:, h] != pick) & ~excused
                if miss.any():
                    bad.append(f"stochastic head {h}: {int(miss.sum())} picks differ from the inverse CDF")
            if e.nvec[h] == 1 and (sa[:, h] != 0).any():
                bad.append(f"size-1 head {h} sampled a nonzero action")
            if e.derived == "sharp":
                got = pr[np.arange(len(a)), np.clip(sa[:, h].astype(np.int64), 0, e.nvec[h] - 1)]
                if (got < 1e-30).any():
                    bad.append(f"sharp: head {h} sampled {int((got < 1e-30).sum())} categories of probability below 1e-30")
            want += np.log(pr[np.arange(len(a)), pick])
        for s in range(e.n_shoot):
            p = ref["shoot_p"][:, s]
            fire = (u[:, n_cat + s] >= 1.0 - p).astype(np.float64)
            excused |= np.abs(u[:, n_cat + s] - (1.0 - p)) < EDGE
            miss = (sa[:, n_cat + s] != fire) & ~excused
            if miss.any():
                bad.append(f"stochastic munition head {s}: {int(miss.sum())} differ")
            pc = np.clip(p, 2.0 ** -23, 1.0 - 2.0 ** -23)   # torch's Bernoulli(probs) clamps p
            want += np.where(fire > 0, np.log(pc), np.log1p(-pc))
        if len(ones) == n_cat and not e.n_shoot and (call["lp"] != 0.0).any():
            bad.append("only size-1 heads, but a stochastic log-prob is not exactly 0")
        hold("slogp", np.abs(call["lp"][:, 0] - want)[~excused].max(), b["slogp"])
    used["excused"] = float(excused.mean())
    return bad, used


# ---- the second restatement: one planted fault at a time
FAULTS = ("drop_last_column", "padding_leak", "head_shift", "unbiased_variance", "last_maximum", "ge_target", "softplus_no_threshold",
          "prior_columns")


def fault_acts(fault, e):
    """Whether a planted fault changes anything at an entry (reasoned from the fault, not from the comparison's verdict)."""
    dims = (e.obs_dim, critic_dim(e))
    return {"drop_last_column": True,                                            # every entry has a last column
            "padding_leak": e.fn and any(d % 32 for d in dims),                  # a padding column exists, and the norm's sums see it
            "head_shift": any(k > 1 for k in e.nvec),                            # size-1 heads give action 0, log-prob 0 wherever they read
            "unbiased_variance": e.fn and any(d > 1 for d in dims),
            "last_maximum": e.derived == "ties",
            "ge_target": e.derived == "ties",                                    # needs a running sum exactly on the target
            "softplus_no_threshold": e.n_shoot > 0,                              # float32 exp overflows past 88: the outer softplus sits near 100
            "prior_columns": e.n_shoot > 0}[fault]


def _t(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64))


def _ln(x, w, b):
    m = x.mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(((x - m) ** 2).mean(-1, keepdim=True) + 1e-5) * w + b


def _trunk(sd, x_in, rnn, masks, fn, fault):
    x = _t(x_in)
    D = x.shape[-1]
    w1 = _t(sd["base.mlp.fc.0.weight"]).clone()
    if fn:
        m = x.mean(-1, keepdim=True)
        ss = ((x - m) ** 2).sum(-1, keepdim=True)
        var = ss / D
        if fault == "padding_leak" and D % 32:   # column D holds the next row's first value, and the sums run over it
            nxt = torch.cat([x[1:, :1], torch.zeros(1, 1, dtype=x.dtype)])
            m = (x.sum(-1, keepdim=True) + nxt) / D
            var = (((x - m) ** 2).sum(-1, keepdim=True) + (nxt - m) ** 2) / D
        if fault == "unbiased_variance" and D > 1:
            var = ss / (D - 1)
        x = (x - m) / torch.sqrt(var + 1e-5) * _t(sd["base.feature_norm.weight"]) + _t(sd["base.feature_norm.bias"])
    if fault == "drop_last_column":
        w1[:, -1] = 0.0
    x = torch.relu(x @ w1.T + _t(sd["base.mlp.fc.0.bias"]))
    x = _ln(x, _t(sd["base.mlp.fc.2.weight"]), _t(sd["base.mlp.fc.2.bias"]))
    x = torch.relu(x @ _t(sd["base.mlp.fc.3.weight"]).T + _t(sd["base.mlp.fc.3.bias"]))
    x = _ln(x, _t(sd["base.mlp.fc.5.weight"]), _t(sd["base.mlp.fc.5.bias"]))
    h = _t(rnn).reshape(-1, 128) * _t(masks).reshape(-1, 1)
    gi = x @ _t(sd["rnn.gru.weight_ih_l0"]).T + _t(sd["rnn.gru.bias_ih_l0"])
    gh = h @ _t(sd["rnn.gru.weight_hh_l0"]).T + _t(sd["rnn.gru.bias_hh_l0"])
    r = torch.sigmoid(gi[:, :128] + gh[:, :128])
    z = torch.sigmoid(gi[:, 128:256] + gh[:, 128:256])
    n = torch.tanh(gi[:, 256:] + r * gh[:, 256:])
    hn = (1 - z) * n + z * h
    return _ln(hn, _t(sd["rnn.norm.weight"]), _t(sd["rnn.norm.bias"])), hn


def _mlp(sd, pre, x):
    for i in (0, 3):
        x = torch.relu(x @ _t(sd[f"{pre}{i}.weight"]).T + _t(sd[f"{pre}{i}.bias"]))
        x = _ln(x, _t(sd[f"{pre}{i + 2}.weight"]), _t(sd[f"{pre}{i + 2}.bias"]))
    return x


def _softplus32(x, threshold):
    x = x.float()
    y = torch.log1p(torch.exp(x))
    return (torch.where(x > 20.0, x, y) if threshold else y).double()


def faulty(name, fault=None):
    """The restatement written out again with ``fault`` planted (None: no fault, equal to policy_util's to rounding)."""
    e, d = ENTRIES[name], inputs(name)
    sd, n_cat = d["sd"], len(e.nvec)
    x, hn = _trunk(sd, d["obs"], d["rnn_states"], d["masks"], e.fn, fault)
    x = _mlp(sd, "act.mlp.fc.", x)
    flat = torch.cat([x @ _t(sd[f"act.action_outs.{i}.logits_net.weight"]).T + _t(sd[f"act.action_outs.{i}.logits_net.bias"])
                      for i in range(n_cat)] + [torch.zeros(len(x), 1, dtype=torch.float64)], -1)
    shift = 1 if fault == "head_shift" else 0
    logits = [flat[:, sl.start + shift:sl.stop + shift] for sl in head_slices(e)]
    acts, lps = [], []
    for l in logits:
        am = l.shape[-1] - 1 - l.flip(-1).argmax(-1) if fault == "last_maximum" else l.argmax(-1)
        acts.append(am.double())
        lps.append(torch.log_softmax(l, -1).gather(-1, am[:, None])[:, 0])
    out = {"logits": torch.cat(logits, -1).numpy(), "probs": torch.cat([torch.softmax(l, -1) for l in logits], -1).numpy()}
    if e.n_shoot:
        o = _t(d["obs"])
        ca, cd = (10, 12) if fault == "prior_columns" else (11, 13)
        ang, dist = torch.rad2deg(o[:, ca]), o[:, cd] * 10000
        a0 = torch.where(dist <= 8000, 10.0, torch.where(dist <= 12000, 6.0, 3.0)).double()
        b0 = torch.where(ang <= 22.5, 3.0, torch.where(ang <= 45, 6.0, 10.0)).double()
        ps = []
        for s in range(e.n_shoot):
            z = x @ _t(sd[f"act.action_outs.{n_cat + s}.net.weight"]).T + _t(sd[f"act.action_outs.{n_cat + s}.net.bias"])
            y = 100 - torch.nn.functional.softplus(100 - torch.nn.functional.softplus(z))
            if fault == "softplus_no_threshold":   # what float32 makes of log1p(exp(x)) past the threshold, as a difference
                y = y + (100 - _softplus32(100 - _softplus32(z, False), False)) - (100 - _softplus32(100 - _softplus32(z, True), True))
            al, be = 1 + y[:, 0], 1 + y[:, 1]
            p = (al + a0) / (al + a0 + be + b0)
            ps.append(p)
            fire = p > 0.5
            acts.append(fire.double())
            pc = p.clamp(2.0 ** -23, 1 - 2.0 ** -23)
            lps.append(torch.where(fire, torch.log(pc), torch.log1p(-pc)))
        out["shoot_p"] = torch.stack(ps, -1).numpy()
    out["actions"] = torch.stack(acts, -1).numpy()
    out["log_probs"] = torch.stack(lps, -1).sum(-1, keepdim=True).numpy()
    out["rnn_states_out"] = hn[:, None, :].numpy()
    csd = d["critic_sd"]
    xc, hc = _trunk(csd, critic_input(e, d), d["rnn_states_critic"], d["masks"], e.fn, fault)
    xc = _mlp(csd, "mlp.fc.", xc)
    out["values"] = (xc @ _t(csd["value_out.weight"]).T + _t(csd["value_out.bias"])).numpy()
    out["rnn_states_critic_out"] = hc[:, None, :].numpy()
    return out


def sample_f32(e, r, u, fault=None):
    """The kernel's sampler on a restatement's logits / p, in float32: (actions, log-probs [N, 1]). ``ge_target`` plants ``c >= target``."""
    lg = r["logits"].astype(np.float32)
    n = len(lg)
    acts, lp = [], np.zeros(n, np.float32)
    for h, sl in enumerate(head_slices(e)):
        x = lg[:, sl]
        ex = np.exp(x - x.max(-1, keepdims=True)).astype(np.float32)
        s = np.zeros(n, np.float32)
        for j in range(ex.shape[1]):
            s = s + ex[:, j]
        target = u[:, h].astype(np.float32) * s
        c, pick, last = np.zeros(n, np.float32), np.full(n, -1), np.zeros(n, np.int64)
        for j in range(ex.shape[1]):
            last = np.where(ex[:, j] > 0, j, last)
            c = c + ex[:, j]
            hit = (c >= target) if fault == "ge_target" else (c > target)
            pick = np.where((pick < 0) & hit, j, pick)
        pick = np.where(pick < 0, last, pick)
        acts.append(pick.astype(np.float64))
        lp = lp + (np.log(ex[np.arange(n), pick]) - np.log(s)).astype(np.float32)
    for k in range(e.n_shoot):
        p = r["shoot_p"][:, k].astype(np.float32)
        fire = u[:, len(e.nvec) + k].astype(np.float32) >= np.float32(1.0) - p
        pc = np.clip(p, np.float32(2.0 ** -23), np.float32(1.0 - 2.0 ** -23))
        acts.append(fire.astype(np.float64))
        lp = lp + np.where(fire, np.log(pc), np.log1p(-pc)).astype(np.float32)
    return np.stack(acts, -1), lp.astype(np.float64)[:, None]


def as_device(e, r, us, fault=None):
    """A restatement's outputs in the shape compare() takes from the device."""
    dev = {"v": r["values"], "a": r["actions"], "lp": r["log_probs"], "ha": r["rnn_states_out"], "hc": r["rnn_states_critic_out"], "stoch": []}
    for u in us:
        a, lp = sample_f32(e, r, u, fault)
        dev["stoch"].append({"u": u, "a": a, "lp": lp})
    return dev
