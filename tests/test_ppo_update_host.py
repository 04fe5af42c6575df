"""The update's tail on the device, without a GPU: the tests' float64 restatements of the loss, the clip and Adam against
tests/golden/ppo_update.npz (the reference's own PPOTrainer.ppo_update, PPO and MAPPO, three consecutive updates), what the cases
cover, the exported names and C ABI symbols, and every refusal that returns before touching a device."""
import copy
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import mlp_train_util as MU
import ppo_update_util as U

torch = pytest.importorskip("torch")
nn = torch.nn


@pytest.fixture(scope="module")
def Pu(pkg):
    return importlib.import_module("aircombat-selfplay_amd.ppo_update")


@pytest.mark.parametrize("algo", ["ppo", "mappo"])
def test_float64_restatement_matches_golden(algo):
    g = U.golden()
    policy, state = U.StubPolicy(torch.float64), {}
    for step in range(U.STUB_STEPS):
        ret = U.restated_update(policy, state, U.stub_sample(step, algo == "mappo"))
        for k in U.RETURNED:
            ref = float(g[f"{algo}/{step}/{k}"])
            assert abs(ret[k] - ref) <= 1e-12 * abs(ref), (algo, step, k, ret[k], ref)
        for name, p in policy.params().items():
            for what, mine in (("", p.detach().numpy()), ("@exp_avg", state[name]["m"]), ("@exp_avg_sq", state[name]["v"])):
                ref = g[f"{algo}/{step}/{name}{what}"]
                assert mine.shape == ref.shape
                assert np.abs(mine - ref).max() <= 1e-12 * np.abs(ref).max(), (algo, step, name, what)
    assert {k.split("/")[0] for k in g} == {"ppo", "mappo"}


def test_golden_is_data_and_no_larger_than_the_mlp_one():
    assert os.path.getsize(U.GOLDEN) <= os.path.getsize(MU.GOLDEN)
    assert all(v.dtype == np.float64 for v in U.golden().values())


def test_cases_cover_what_they_claim():
    g, clip = U.golden(), U.ARGS["clip_param"]
    for algo in ("ppo", "mappo"):   # one group clipped, the other not, in every update
        for step in range(U.STUB_STEPS):
            assert float(g[f"{algo}/{step}/actor_grad_norm"]) < U.ARGS["max_grad_norm"] < float(g[f"{algo}/{step}/critic_grad_norm"])
    t65 = U.loss_inputs(65, 65)
    for M in (63, 65, 1025):
        t = U.loss_inputs(M, M)
        ratio = np.exp(t["action_log_probs"].astype(np.float64) - t["old_action_log_probs"])
        d = t["values"].astype(np.float64) - t["value_preds"]
        assert (ratio < 1 - clip).any() and (ratio > 1 + clip).any() and ((ratio > 1 - clip) & (ratio < 1 + clip)).any()
        assert (d < -clip).any() and (d > clip).any() and (np.abs(d) < clip).any()
        assert (t["advantages"] == 0).any() and (t["advantages"] > 0).any() and (t["advantages"] < 0).any()
        assert (t["action_log_probs"] == t["old_action_log_probs"]).any() and (t["values"] == t["value_preds"]).any()
        assert (t["active_masks"] == 0).any() and (t["active_masks"] == 1).any()
    three = U.loss_inputs(65, 65, old_cols=3)
    assert three["old_action_log_probs"].shape == (65, 3) and (three["old_action_log_probs"][:, 0] == t65["old_action_log_probs"][:, 0]).all()
    one = U.loss_inputs(1, 1)
    assert one["values"].shape == (1, 1) and one["active_masks"][0, 0] == 1


def test_restated_gradient_conventions():
    """What autograd decides and the kernel restates: clamp passes the gradient on its closed interval, min / max split a tie."""
    x = torch.tensor([0.8, 1.2, 0.5, 1.0], dtype=torch.float64, requires_grad=True)
    torch.clamp(x, 0.8, 1.2).sum().backward()
    assert x.grad.tolist() == [1.0, 1.0, 0.0, 1.0]
    a, b = torch.tensor([1.0, 2.0], dtype=torch.float64, requires_grad=True), torch.tensor([1.0, 3.0], dtype=torch.float64, requires_grad=True)
    torch.min(a, b).sum().backward()
    assert a.grad.tolist() == [0.5, 1.0] and b.grad.tolist() == [0.5, 0.0]


def test_clip_and_adam_restatements_match_torch():
    """clip_adam_f64 against clip_grad_norm_ + torch.optim.Adam in float64 on the CPU, three steps, one group clipped."""
    ps = [nn.Parameter(torch.tensor(np.float64(0.3) * np.arange(1, 6))), nn.Parameter(torch.tensor(np.linspace(-1, 1, 7)))]
    opt = torch.optim.Adam([{"params": [ps[0]]}, {"params": [ps[1]]}], lr=U.LR, eps=U.ADAM_EPS)
    state, mine = {}, [p.detach().numpy().copy() for p in ps]
    for step in range(3):
        grads = [np.cos(np.arange(5) + step) * 0.01, np.sin(np.arange(7) + step) * 100.0]
        for p, g in zip(ps, grads):
            p.grad = torch.tensor(g)
        tn = [float(nn.utils.clip_grad_norm_([p], 2.0)) for p in ps]
        opt.step()
        norms, new_p, new_g = U.clip_adam_f64([[(0, mine[0], grads[0])], [(1, mine[1], grads[1])]], state, 2.0)
        mine = [new_p[0], new_p[1]]
        assert norms[0] < 2.0 < norms[1] and np.allclose(norms, tn, rtol=1e-14)
        for i, p in enumerate(ps):
            assert np.abs(mine[i] - p.detach().numpy()).max() <= 1e-14, (step, i)
            assert np.abs(new_g[i] - p.grad.numpy()).max() <= 1e-14 * np.abs(new_g[i]).max()
            assert np.allclose(state[i]["m"], opt.state[p]["exp_avg"].numpy(), rtol=1e-13, atol=0)
            assert np.allclose(state[i]["v"], opt.state[p]["exp_avg_sq"].numpy(), rtol=1e-13, atol=0)
    assert np.isnan(U.clip_coef(float("nan"), 2.0)) and U.clip_coef(0.0, 2.0) == 1.0 and U.clip_coef(float("inf"), 2.0) == 0.0


def test_exports_and_symbols(pkg, Pu):
    for name in ("ppo_loss", "device_clip_adam_step", "DevicePPOTrainer", "DevicePPOLossFunction"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(Pu, name)
    lib = pkg.load_library()
    for sym in ("ac_ppo_loss_workspace_floats", "ac_ppo_loss_forward", "ac_ppo_loss_backward", "ac_optim_workspace_floats",
                "ac_optim_grad_norms", "ac_optim_clip_adam_step"):
        assert sym in pkg.capi.SIGNATURES and hasattr(lib, sym)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aircombat.h")).read()
    assert "ac_optim_entry_t" in header
    c = Pu.constants()
    assert c["max_entries"] >= 512 and c["loss_rows"] >= 64 and c["chunk"] >= 128
    assert C.sizeof(pkg.capi.AcOptimEntry) == Pu._ENTRY.itemsize == 96
    t = Pu.DevicePPOTrainer(U.trainer_args(), torch.device("cpu"))
    assert (t.ppo_epoch, t.clip_param, t.max_grad_norm, t.data_chunk_length) == (2, 0.2, 2.0, 8) and not t.use_policy_active_masks
    assert Pu.DevicePPOTrainer.KEYS == ("value_loss", "policy_loss", "policy_entropy_loss", "actor_grad_norm", "critic_grad_norm", "ratio")


def _table(pkg, n, **over):
    tab = (pkg.capi.AcOptimEntry * max(n, 1))()
    for i in range(n):
        tab[i].p = tab[i].g = tab[i].m = tab[i].v = 16   # never dereferenced: every call below is refused before it touches a device
        tab[i].numel, tab[i].group = 5, i % 2
        tab[i].lr, tab[i].eps, tab[i].beta1, tab[i].beta2, tab[i].bias_correction1, tab[i].bias_correction2 = 5e-4, 1e-5, 0.9, 0.999, 0.1, 0.001
    for k, v in over.items():
        setattr(tab[0], k, v)
    return tab


def test_capi_refusals(pkg):
    lib = pkg.load_library()
    p = 16   # never dereferenced
    err = lambda: lib.last_error()

    def fwd(M, n_ent=4, null=None, cols=1):
        a = [p] * 6 + [None, p] + [p] * 5   # logp old adv values vpreds returns | active ent | ws stats loss dlogp dvalues
        if null is not None:
            a[null] = None
        return lib.ac_ppo_loss_forward(0, None, M, n_ent, cols, *a[:8], 0.2, 1.0, 0.01, 1, *a[8:])
    for null in (0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12):   # active (6) and d_loss (10) may be NULL
        assert fwd(4, null=null) == -1 and "null argument" in err(), null
    for M, n_ent, what in ((0, 4, "M must be at least 1"), (-3, 4, "M must be at least 1"), (4, 0, "n_ent must be at least 1"),
                           (2 ** 31 - 1, 4, "32-bit index")):
        assert fwd(M, n_ent) == -1 and what in err(), (M, err())
        assert lib.ac_ppo_loss_workspace_floats(M, n_ent) == -1 and what in err()
        assert lib.ac_ppo_loss_backward(0, None, M, n_ent, p, p, p, 0.01, p, p, p) == -1 and what in err()
    for cols in (0, 65):
        assert fwd(4, cols=cols) == -1 and "old_cols must be 1 .. 64" in err()
    for null in (0, 1, 2):
        a = [p, p, p]
        a[null] = None
        assert lib.ac_ppo_loss_backward(0, None, 4, 4, *a, 0.01, p, p, p) == -1 and "null argument" in err()
    rows, wgs = lib.ac_ppo_update_constant(0), lib.ac_ppo_update_constant(1)
    assert lib.ac_ppo_loss_workspace_floats(1, 1) == 5 and lib.ac_ppo_loss_workspace_floats(rows + 1, 1) == 10
    assert lib.ac_ppo_loss_workspace_floats(rows * wgs * 3, 1) == 5 * wgs

    # ---- the optimiser's table
    chunk, cap = lib.ac_ppo_update_constant(2), lib.ac_ppo_update_constant(3)
    layout = lambda tab, n, ng=2: lib.ac_optim_workspace_floats(tab, n, ng)
    norms = lambda tab, n, ng=2, d=p, ws=p, out=p: lib.ac_optim_grad_norms(0, None, tab, d, n, ng, ws, out)
    step = lambda tab, n, ng=2, d=p, nr=p: lib.ac_optim_clip_adam_step(0, None, tab, d, n, ng, nr, 2.0, 1)
    for call in (layout, norms, step):
        assert call(None, 1) == -1 and "null argument" in err()
        assert call(_table(pkg, 0), 0) == -1 and "no entries" in err()
        assert call(_table(pkg, cap + 1), cap + 1) == -1 and f"{cap + 1} entries (at most {cap})" in err()
        assert call(_table(pkg, 2, numel=0), 2) == -1 and "entry 0: numel must be at least 1" in err()
        assert call(_table(pkg, 2, group=2), 2) == -1 and "entry 0: group 2 out of range" in err()
        assert call(_table(pkg, 2, group=-1), 2) == -1 and "out of range" in err()
        assert call(_table(pkg, 2, g=None), 2) == -1 and "entry 0: null pointer" in err()
        assert call(_table(pkg, 2, m=18), 2) == -1 and "4-byte aligned" in err()
        assert call(_table(pkg, 2), 2, 0) == -1 and "n_groups" in err()
    tab = _table(pkg, 3, numel=2 * chunk + 1)
    assert norms(tab, 3) == -1 and "first_chunk" in err()   # not laid out yet
    assert layout(tab, 3) == 2 * (3 + 1 + 1) and [e.first_chunk for e in tab] == [0, 3, 4]
    assert norms(tab, 3, d=None) == -1 and "null argument" in err()
    assert norms(tab, 3, out=None) == -1 and "null argument" in err()
    assert step(tab, 3, nr=None) == -1 and "null argument" in err()
    assert layout(_table(pkg, cap), cap) == 2 * cap   # the table's full size is accepted


def test_ppo_loss_refuses_cpu_tensors_and_shapes(Pu, pkg):
    t = {k: torch.as_tensor(v) for k, v in U.loss_inputs(8, 8).items()}
    args = lambda **o: [{**t, **o}[k] for k in ("values", "action_log_probs", "dist_entropy", "old_action_log_probs", "advantages", "returns", "value_preds")]
    kw = dict(clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01)
    with pytest.raises(pkg.UnsupportedPolicy, match="float32 on one CUDA device"):
        Pu.ppo_loss(*args(), **kw)
    with pytest.raises(pkg.UnsupportedPolicy, match="float64"):
        Pu.ppo_loss(*args(values=t["values"].double()), **kw)
    with pytest.raises(ValueError, match=r"expected \[M, 1\]"):
        Pu.ppo_loss(*args(action_log_probs=t["action_log_probs"].view(-1)), **kw)
    with pytest.raises(ValueError, match=r"expected \[M, 1\]"):
        Pu.ppo_loss(*args(action_log_probs=t["action_log_probs"].numpy()), **kw)


def _adam(**kw):
    ps = [nn.Parameter(torch.arange(6.0).view(2, 3)), nn.Parameter(torch.ones(4))]
    for p in ps:
        p.grad = torch.full_like(p, 0.5)
    return torch.optim.Adam([{"params": ps[:1]}, {"params": ps[1:]}], lr=1e-3, **kw), ps


@pytest.mark.parametrize("what,make", [
    ("SGD", lambda: (torch.optim.SGD(_adam()[1], lr=0.1), None)),
    ("AdamW", lambda: (torch.optim.AdamW(_adam()[1], lr=0.1, weight_decay=0.0), None)),
    ("amsgrad", lambda: _adam(amsgrad=True)),
    ("weight_decay", lambda: _adam(weight_decay=0.01)),
    ("maximize", lambda: _adam(maximize=True)),
    ("differentiable", lambda: _adam(differentiable=True)),
    ("only a CUDA device", lambda: _adam()),
])
def test_device_step_refusals_change_nothing(Pu, pkg, what, make):
    opt, _ = make()
    params = [p for g in opt.param_groups for p in g["params"]]
    if what == "differentiable":
        params = [p.detach() for p in params]
    before = [p.detach().clone() for p in params]
    grads = [None if p.grad is None else p.grad.clone() for p in params]
    sd = copy.deepcopy(opt.state_dict())
    with pytest.raises(pkg.UnsupportedPolicy, match=what):
        Pu.device_clip_adam_step(opt, 2.0)
    assert len(opt.state) == 0 and opt.state_dict() == sd
    for p, b, g in zip(params, before, grads):
        assert torch.equal(p.detach(), b) and (g is None or torch.equal(p.grad, g))


def test_device_step_refuses_with_existing_state_untouched(Pu, pkg):
    opt, ps = _adam()
    opt.step()
    snap = {k: (v["step"].clone(), v["exp_avg"].clone(), v["exp_avg_sq"].clone()) for k, v in opt.state.items()}
    before = [p.detach().clone() for p in ps]
    opt.param_groups[1]["capturable"] = True
    with pytest.raises(pkg.UnsupportedPolicy, match="capturable=True"):
        Pu.device_clip_adam_step(opt, 2.0)
    for p, b in zip(ps, before):
        assert torch.equal(p.detach(), b)
        s = opt.state[p]
        assert float(s["step"]) == 1 and torch.equal(s["exp_avg"], snap[p][1]) and torch.equal(s["exp_avg_sq"], snap[p][2])
    d = nn.Parameter(torch.zeros(3, dtype=torch.float64))
    d.grad = torch.ones(3, dtype=torch.float64)
    with pytest.raises(pkg.UnsupportedPolicy, match="float64"):
        Pu.device_clip_adam_step(torch.optim.Adam([d]), 2.0)
    nc = nn.Parameter(torch.zeros(3, 4).t())
    nc.grad = torch.ones(4, 3)
    with pytest.raises(pkg.UnsupportedPolicy, match="non-contiguous parameter"):
        Pu.device_clip_adam_step(torch.optim.Adam([nc]), 2.0)


def test_trainer_refuses_other_samples_and_groups(Pu, pkg):
    tr = Pu.DevicePPOTrainer(U.trainer_args(), torch.device("cpu"))
    with pytest.raises(ValueError, match="9"):
        tr.ppo_update(U.StubPolicy(torch.float32), (1, 2, 3))
    pol = U.StubPolicy(torch.float32)
    pol.optimizer = torch.optim.Adam(list(pol.actor.parameters()) + list(pol.critic.parameters()))
    with pytest.raises(pkg.UnsupportedPolicy, match="param groups"):
        tr.ppo_update(pol, U.stub_sample(0, False))
    with pytest.raises(NotImplementedError):
        Pu.DevicePPOTrainer(U.trainer_args(use_recurrent_policy=False), torch.device("cpu")).train(pol, None)
