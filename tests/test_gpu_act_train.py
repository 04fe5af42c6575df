"""The training action heads (use_device_act, csrc/act_train.hpp) on the MI355X: against the reference's float64 ACTLayer
(tests/golden/act_train.npz), against float64 torch at a user's size, inside a whole PPO update with the GRU and the MLP layers swapped
too, and their determinism, stream and sync discipline, refusals and behaviour on bad actions.

The bound everywhere: with rel(a, ref) = max|a - ref| / max|ref| against float64, rel(device) <= max(4 * rel(torch fp32 eager on the
same GPU), 2^-20), the bound test_gpu_mlp_train.py and test_gpu_gru_train.py use for the same kind of comparison."""
import copy
import ctypes as C
import importlib
import math
import types

import numpy as np
import pytest

import act_train_util as U
import mlp_train_util as MU

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
nn = torch.nn
FLOOR = 2.0 ** -20


@pytest.fixture(scope="module")
def At(pkg):
    return importlib.import_module("aircombat-selfplay_amd.act_train")


@pytest.fixture(scope="module")
def Mt(pkg):
    return importlib.import_module("aircombat-selfplay_amd.mlp_train")


@pytest.fixture(scope="module")
def Gt(pkg):
    return importlib.import_module("aircombat-selfplay_amd.gru_train")


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def run(case, inp, At=None, dtype=torch.float32):
    """(results, indices of the heads without a gradient) of a case on the GPU: the eager module, or with ``At`` the device path."""
    m = U.act_from(case, inp, "cuda", dtype)
    if At is not None:
        assert At.use_device_act(m) == 1
    x = torch.as_tensor(inp["x"]).to("cuda", dtype).requires_grad_(True)
    return U.run_with_grads(m.evaluate_actions, dict(m.named_parameters()), x, inp, case)


def compare(what, case, dev, ref, gold):
    bad = []
    for k in U.keys(case):
        assert np.isfinite(dev[k]).all(), (what, k)
        e_dev, e_ref = rel(dev[k], gold[k]), rel(ref[k], gold[k])
        print(f"{what} {k}: device {e_dev:.2e}, torch fp32 {e_ref:.2e}")
        if not e_dev <= max(4 * e_ref, FLOOR):
            bad.append((k, e_dev, e_ref))
    assert not bad, (what, bad)


@pytest.mark.parametrize("name", list(U.CASES))
def test_golden_agreement(At, name):
    g, inp = U.golden(), U.inputs(name)
    (dev, dev_unused), (ref, ref_unused) = run(name, inp, At), run(name, inp)
    assert set(dev) == set(U.keys(name))
    compare(f"golden {name}", name, dev, ref, {k: g[f"{name}/{k}"] for k in U.keys(name)})
    assert dev["logp"].shape == dev["ent"].shape == (U.CASES[name][0], 1)
    # the munition heads the reference leaves out get no gradient on either path
    assert dev_unused == ref_unused == [i for i in range(U.n_heads(name)) if i not in U.used_heads(name)]
    if name in ("shoot4", "sharp"):
        assert dev_unused == [3, 4, 5]
    if U.CASES[name][3]:   # inactive rows change nothing but the scaling
        free = {k: v for k, v in inp.items() if k != "active_masks"}
        (unm, _), am, M = run(name, free, At), inp["active_masks"].astype(np.float64), U.CASES[name][0]
        assert np.array_equal(unm["logp"], dev["logp"])
        assert (dev["ent"][am == 0] == 0).all() and (am == 0).any()
        assert np.abs(dev["ent"] * am.sum() - unm["ent"] * M * am).max() <= 2.0 ** -21 * np.abs(unm["ent"] * M).max()


def _big_inputs(case, seed):
    M, nvec, ns, masked = case
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    sizes = list(nvec) + [2] * ns
    inp = {}
    for wn, n in zip(U.pnames(case)[0::2], sizes):
        inp[wn], inp[wn[:-6] + "bias"] = rn(n, 128) / math.sqrt(128), rn(n) * 0.1
    inp.update(x=rn(M, 128), g1=rn(M, 1), g2=rn(M, 1))
    inp["action"] = torch.stack([torch.randint(0, n, (M,), device="cuda", generator=gen) for n in sizes], -1).float()
    if ns:
        pick = lambda vals: torch.tensor(vals, device="cuda")[torch.randint(0, 3, (M, 1), device="cuda", generator=gen)]
        inp.update(alpha0=pick(U.ALPHA0), beta0=pick(U.BETA0))
    if masked:
        inp["active_masks"] = (torch.rand(M, 1, device="cuda", generator=gen) > 0.1).float()
    return {k: v.cpu().numpy() for k, v in inp.items()}


@pytest.mark.parametrize("nvec,ns", [((3, 5, 3), 4), ((41, 41, 41, 30), 0)], ids=["3-5-3+2x4", "41-41-41-30"])
def test_parity_at_user_size(At, nvec, ns):
    """The heads at M = 4096 x 60 rows against the same modules in float64 on the GPU: the parameter gradients are sums over 245 760
    rows here (256 workgroup partials of 960 rows each, then eight interleaved sums and a tree)."""
    case = (4096 * 60, nvec, ns, bool(ns))
    inp = _big_inputs(case, seed=3 + ns)
    (dev, _), (ref, _), (f64, _) = run(case, inp, At), run(case, inp), run(case, inp, dtype=torch.float64)
    compare(f"parity 4096 x 60 {list(nvec)} + {ns}", case, dev, ref, f64)


# ---- a whole PPO update on the restated policy (act_train_util), fed by an on-device minibatch
def _filled_buffer(pkg, shared=False, T=32, E=32, L=8, seed=5):
    OBS, NVEC = MU.OBS, MU.NVEC
    args = types.SimpleNamespace(buffer_size=T, n_rollout_threads=E, gamma=0.99, use_proper_time_limits=False, use_gae=True, gae_lambda=0.95,
                                 recurrent_hidden_size=128, recurrent_hidden_layers=1)
    buf = (pkg.DeviceSharedReplayBuffer(args, 2, OBS, 2 * OBS, len(NVEC)) if shared else pkg.DeviceReplayBuffer(args, 1, OBS, len(NVEC)))
    gen = torch.Generator(device="cuda").manual_seed(seed)
    for name in ("obs", "rewards", "action_log_probs", "value_preds", "rnn_states_actor", "rnn_states_critic") + (("share_obs",) if shared else ()):
        buf.device_tensor(name).normal_(generator=gen)
    buf.device_tensor("action_log_probs").mul_(0.1).sub_(2.0)
    a = buf.device_tensor("actions")
    for i, n in enumerate(NVEC):
        a[..., i] = torch.randint(0, n, a[..., i].shape, device="cuda", generator=gen).float()
    buf.device_tensor("masks").copy_((torch.rand(buf.device_tensor("masks").shape, device="cuda", generator=gen) > 0.05).float())
    if shared:
        buf.device_tensor("active_masks").copy_((torch.rand(buf.device_tensor("active_masks").shape, device="cuda", generator=gen) > 0.1).float())
    nv = torch.randn(E * buf.num_agents, device="cuda", generator=gen)
    torch.cuda.synchronize()   # the buffer's kernels run on its own stream
    buf.compute_returns(nv, on_device=True)
    torch.cuda.synchronize()
    return buf, T * E // L, L


def _flat(ts):
    return torch.cat([t.detach().double().reshape(-1) for t in ts]).cpu().numpy()


@pytest.mark.parametrize("shared", [False, True], ids=["own-obs", "share-obs"])
def test_whole_ppo_update(At, Mt, Gt, pkg, shared):
    buf, nchunks, L = _filled_buffer(pkg, shared=shared, seed=5 + shared)
    order = np.random.default_rng(0).permutation(nchunks)
    gen = buf.recurrent_generator(buf.advantages, 1, L, chunk_order=order, on_device=True) if shared else \
        buf.recurrent_generator(buf, 1, L, chunk_order=order, on_device=True)
    sample = next(gen)
    assert all(isinstance(s, torch.Tensor) and s.is_cuda for s in sample)
    base = U.Policy(seed=11, critic_obs=2 * MU.OBS if shared else MU.OBS)
    runs = {}
    for kind in ("torch", "device", "f64"):
        pol = copy.deepcopy(base)
        if kind == "device":
            adam_params = [p for grp in pol.optimizer.param_groups for p in grp["params"]]
            act = pol.actor.act
            assert Gt.use_device_gru(pol) == 2 and Mt.use_device_mlp(pol) == 4 and At.use_device_act(pol) == 1
            assert pol.actor.act is act and act.evaluate_actions.__func__ is At._device_evaluate_actions
            assert isinstance(act.mlp, Mt.DeviceMLPLayer)
            # the optimiser built before the swaps still holds the very Parameter objects the swapped modules use
            assert [id(p) for p in adam_params] == [id(p) for p in list(pol.actor.parameters()) + list(pol.critic.parameters())]
        s = sample
        if kind == "f64":
            pol.actor.double(); pol.critic.double()
            s = tuple(t.double() for t in sample)
        MU.ppo_update(pol, s, shared=shared)
        params = list(pol.actor.parameters()) + list(pol.critic.parameters())
        runs[kind] = (_flat([p.grad for p in params]), _flat(params))
        if kind == "device":
            st = pol.optimizer.state
            assert all(p in st and "exp_avg" in st[p] for p in params)   # the Adam state lives on the same Parameter objects
    for i, what in enumerate(("gradients", "parameters")):
        e_dev, e_ref = rel(runs["device"][i], runs["f64"][i]), rel(runs["torch"][i], runs["f64"][i])
        assert np.isfinite(runs["device"][i]).all()
        print(f"ppo update ({'share_obs' if shared else 'own obs'}) {what}: device {e_dev:.2e}, torch fp32 {e_ref:.2e}")
        assert e_dev <= max(4 * e_ref, FLOOR), (what, e_dev, e_ref)


def test_determinism(At):
    big = (4096 * 8, (41, 41, 41, 30), 1, True)
    for case, inp in (("wide", U.inputs("wide")), (big, _big_inputs(big, seed=2))):
        (a, _), (b, _) = run(case, inp, At), run(case, inp, At)
        assert set(a) == set(U.keys(case))
        for k in a:
            assert np.array_equal(a[k], b[k]), k


def _on_device(case, inp, At):
    m = U.act_from(case, inp, "cuda")
    assert At.use_device_act(m) == 1
    t = {k: torch.as_tensor(v).cuda() for k, v in inp.items() if not k.startswith("action_outs")}
    prior = {k: t[k] for k in ("alpha0", "beta0") if k in t}
    return m, t, prior


def test_no_host_synchronisation(At):
    case = (512 * 60, (3, 5, 3), 4, True)
    m, t, prior = _on_device(case, _big_inputs(case, seed=4), At)
    x = t["x"].requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        logp, ent = m.evaluate_actions(x, t["action"], t["active_masks"], **prior)
        ((logp * t["g1"]).sum() + (ent * t["g2"]).sum()).backward()
        with pytest.raises(RuntimeError):   # a torch call that does synchronise raises under the same mode: the check is live
            logp.sum().item()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    used = [p for i in U.used_heads(case) for p in m.action_outs[i].parameters()]
    assert torch.isfinite(x.grad).all() and all(torch.isfinite(p.grad).all() for p in used)


def test_side_stream(At):
    inp = U.inputs("shoot1")
    base, _ = run("shoot1", inp, At)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side, _ = run("shoot1", inp, At)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for k in U.keys("shoot1"):
        assert np.array_equal(base[k], side[k]), k


def test_inference_path(At, monkeypatch):
    m, t, prior = _on_device("shoot4", U.inputs("shoot4"), At)
    saves = []
    fwd = At.DeviceActEvalFunction.forward
    monkeypatch.setattr(At.DeviceActEvalFunction, "forward", staticmethod(lambda ctx, *a: (saves.append(a[6]), fwd(ctx, *a))[1]))
    ev = lambda: m.evaluate_actions(t["x"], t["action"], t["active_masks"], **prior)
    lp_grad, ent_grad = ev()
    assert saves == [True] and lp_grad.grad_fn is not None and ent_grad.grad_fn is not None
    with torch.no_grad():
        lp_ng, ent_ng = ev()
    assert saves == [True, False] and lp_ng.grad_fn is None and not ent_ng.requires_grad
    for p in m.parameters():
        p.requires_grad_(False)
    lp_fr, ent_fr = ev()                                 # grad mode on, but nothing requires grad
    assert saves == [True, False, False] and lp_fr.grad_fn is None and ent_fr.grad_fn is None
    assert torch.equal(lp_ng, lp_grad) and torch.equal(lp_fr, lp_grad) and torch.equal(ent_ng, ent_grad) and torch.equal(ent_fr, ent_grad)
    lp_x, _ = m.evaluate_actions(t["x"].clone().requires_grad_(True), t["action"], t["active_masks"], **prior)
    assert saves[-1] is True and lp_x.grad_fn is not None   # frozen heads, but x wants its gradient
    lp_f, ent_f = At.act_evaluate(t["x"], m.action_outs, t["action"], t["active_masks"], **prior)   # the functional form is the same call
    assert torch.equal(lp_f, lp_grad) and torch.equal(ent_f, ent_grad)


def test_refusals_on_the_device(At, pkg):
    inp = U.inputs("shoot4")
    m, t, prior = _on_device("shoot4", inp, At)
    with pytest.raises(KeyError):                        # a tuple space without its priors, as the reference
        m.evaluate_actions(t["x"], t["action"])
    with pytest.raises(pkg.UnsupportedPolicy, match="input torch.float64"):
        m.evaluate_actions(t["x"].double(), t["action"], **prior)
    with pytest.raises(pkg.UnsupportedPolicy, match=r"action_outs\.0\.logits_net: dtype torch.float64"):
        m.double().evaluate_actions(t["x"].double(), t["action"], **prior)
    with pytest.raises(pkg.UnsupportedPolicy, match=r"action_outs\.0\.logits_net: device cpu"):
        m.float().cpu().evaluate_actions(t["x"], t["action"], **prior)
    # the C calls: refused with a message, nothing launched (the outputs keep their sentinel)
    lib = pkg.load_library()
    capi = importlib.import_module("aircombat-selfplay_amd.capi")
    M, nvec = 8, (3, 5, 3)
    f = lambda v, *s: torch.full(s, v, device="cuda")
    x, act, a0, b0 = f(0.5, M, 128), f(0.0, M, 3), f(3.0, M), f(10.0, M)
    ws_ = [f(0.01, n, 128) for n in nvec]
    bs_ = [f(0.0, n) for n in nvec]
    logp, ent, ws, dx = f(-3.0, M), f(-3.0, M), f(-3.0, 129 * 11), f(-3.0, M, 128)
    dws, dbs = [f(-3.0, n, 128) for n in nvec], [f(-3.0, n) for n in nvec]
    g = f(1.0, M)
    outs = [logp, ent, ws, dx] + dws + dbs
    P = lambda v: v.data_ptr()
    arr = lambda ts: (C.c_void_p * len(ts))(*[P(v) for v in ts])
    stream = torch.cuda.current_stream().cuda_stream

    def heads(nv, cols=0):
        h = capi.AcActHeads(n_cat=len(nv), n_shoot_cols=cols)
        h.nvec[:len(nv)] = list(nv)
        return h

    def fwd(h, M, xp=P(x), prior=True):
        return lib.ac_act_eval_forward(0, stream, C.byref(h), M, xp, arr(ws_), arr(bs_), P(act), P(a0) if prior else None, P(b0) if prior else None,
                                       P(logp), P(ent))

    def bwd(h, M, xp=P(x), prior=True):
        return lib.ac_act_eval_backward(0, stream, C.byref(h), M, P(g), P(g), xp, arr(ws_), arr(bs_), P(act), P(a0) if prior else None,
                                        P(b0) if prior else None, P(ws), P(dx), arr(dws), arr(dbs))

    ok = heads(nvec)
    for call in (fwd, bwd):
        for args, what in (((ok, 0), "M must be"), ((heads((3, 1, 3)), M), "at least 2"), ((heads((3, 5, 3), 2), M), "n_shoot_cols must be"),
                           ((heads((80, 80, 3)), M), "at most 160"), ((ok, M, None), "null argument"),
                           ((heads((3, 5), 1), M, P(x), False), "need alpha0 and beta0")):
            assert call(*args) == -1 and what in lib.last_error(), (args, lib.last_error())
    torch.cuda.synchronize()
    assert all(bool((v == -3.0).all()) for v in outs)
    assert fwd(ok, M) == 0 and bwd(ok, M) == 0        # and the same buffers are accepted when the arguments are in range
    torch.cuda.synchronize()
    # equal logits in every head and action 0 everywhere: logp = -log 45, ent = log 45
    assert torch.allclose(logp, f(-math.log(45.0), M), rtol=1e-6) and torch.allclose(ent, f(math.log(45.0), M), rtol=1e-6)
    assert all(torch.isfinite(v).all() and not bool((v == -3.0).any()) for v in outs)


def test_bad_actions(At):
    """One row of ``small`` is given action 7 in a head of 3 and one 1.5: those rows' logp are NaN, everything else of the forward and
    every other row's dx are bit-equal to the clean run's. In the backward a bad action matches no logit, so with those two rows'
    upstream gradients zero the parameter gradients are bit-equal to the clean run's under the same upstream gradients (the rows
    contribute +0 to every sum), and agree with a run on the other 75 rows alone to summation-order rounding."""
    clean = U.inputs("small")
    M, rows = U.CASES["small"][0], [5, 40]
    keep = np.setdiff1d(np.arange(M), rows)
    bad = dict(clean, action=clean["action"].copy())
    bad["action"][5, 0], bad["action"][40, 1] = 7.0, 1.5
    (c, _), (b, _) = run("small", clean, At), run("small", bad, At)
    assert np.isnan(b["logp"][rows]).all() and np.isfinite(b["logp"][keep]).all()
    assert np.array_equal(b["logp"][keep], c["logp"][keep]) and np.array_equal(b["ent"], c["ent"])
    assert np.array_equal(b["dx"][keep], c["dx"][keep]) and np.isfinite(b["dx"]).all()
    zero = lambda d: dict(d, **{k: np.where(np.isin(np.arange(M), rows)[:, None], np.float32(0), d[k]) for k in ("g1", "g2")})
    (cz, _), (bz, _) = run("small", zero(clean), At), run("small", zero(bad), At)
    pk = [k for k in U.keys("small") if k[0] == "d" and k != "dx"]
    assert len(pk) == 6
    for k in pk + ["dx"]:
        assert np.array_equal(bz[k], cz[k]) and np.isfinite(bz[k]).all(), k
    assert (bz["dx"][rows] == 0).all()
    # without those rows at all: M = 75, so dist_entropy's 1 / M is undone through g2
    fewer = {k: (v[keep] if k in ("x", "action", "g1", "g2") else v) for k, v in clean.items()}
    fewer["g2"] = fewer["g2"] * np.float32(len(keep) / M)
    (fw, _) = run((len(keep), (3, 5, 3), 0, False), fewer, At)
    for k in pk:
        assert rel(fw[k], bz[k]) <= 2.0 ** -20, (k, rel(fw[k], bz[k]))
