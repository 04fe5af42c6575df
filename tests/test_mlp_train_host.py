"""The training MLP blocks without a GPU: the tests' float64 restatement of the reference's MLPLayer against tests/golden/mlp_train.npz,
use_device_mlp on a CPU copy of the restated policy (what it finds, keeps and refuses, and how it composes with use_device_gru), and
the C ABI refusals that return before touching a device."""
import importlib

import numpy as np
import pytest

import mlp_train_util as U

torch = pytest.importorskip("torch")
nn = torch.nn


def _f64_case(name):
    inp = U.inputs(name)
    p = {k: torch.tensor(inp[k], dtype=torch.float64, requires_grad=True) for k in U.PNAMES}
    x = torch.tensor(inp["x"], dtype=torch.float64, requires_grad=U.CASES[name][2])
    return U.run_with_grads(lambda x: U.layer(p, x), p, x, torch.tensor(inp["g_out"], dtype=torch.float64))


@pytest.mark.parametrize("name", list(U.CASES))
def test_float64_restatement_matches_golden(name):
    g = U.golden()
    res = _f64_case(name)
    assert set(res) == set(U.keys(name))
    assert {k for k in g if k.startswith(name + "/") and "@" not in k} == {f"{name}/{k}" for k in U.keys(name)}
    for k in U.keys(name):
        s = U.stored(k, res[k])
        ref = g[f"{name}/{k}"]
        assert s.shape == ref.shape, (k, s.shape, ref.shape)
        # the float64 projection to 1e-12, every element to the float32 storage's rounding
        p, rp = U.project(k, s), float(g[f"{name}/{k}@p"])
        scale = float(np.abs(s.ravel()) @ np.abs(U.projector(k, s.size)))
        assert abs(p - rp) <= 1e-12 * scale, (name, k, p, rp)
        assert np.abs(s - ref).max() <= 2.0 ** -23 * np.abs(s).max() + 1e-30, (name, k)


def test_cases_cover_what_they_are_for():
    assert all(U.CASES["wide"][0] % t for t in (16, 32, 64, 128)) and U.CASES["wide"][1] == 128
    assert U.CASES["obs15"][1] % 4 and not U.CASES["obs15"][2] and "dx0" not in U.keys("obs15")
    assert 128 < U.CASES["share"][1] <= 256 and U.CASES["one"][0] == 1
    inp = U.inputs("dead")
    dead = list(U.DEAD_ROWS)
    z = inp["x"].astype(np.float64) @ inp["fc.0.weight"].astype(np.float64).T + inp["fc.0.bias"]
    assert (z[dead] <= 0).all() and (z[dead] == 0).any()                       # relu(z) all zero on the dead rows, with ties at 0
    live = np.setdiff1d(np.arange(U.CASES["dead"][0]), dead)
    assert ((z[live] > 0).sum(axis=1) > 8).all()                               # and the other rows are ordinary
    gam = inp["fc.2.weight"]
    assert (gam == 0).any() and (gam < 0).any() and (gam > 0).any()
    res = _f64_case("dead")
    assert np.array_equal(res["y0"][dead], np.broadcast_to(inp["fc.2.bias"].astype(np.float64), (len(dead), 128)))   # y = beta exactly
    assert all(np.isfinite(v).all() for v in res.values())
    for name in U.CASES:                                                       # gamma and beta are hashed everywhere, not 1 and 0
        i = U.inputs(name)
        assert all(np.unique(i[k]).size > 64 for k in ("fc.2.weight", "fc.2.bias", "fc.5.weight", "fc.5.bias"))


@pytest.fixture(scope="module")
def Mt(pkg):
    return importlib.import_module("aircombat-selfplay_amd.mlp_train")


@pytest.fixture(scope="module")
def Gt(pkg):
    return importlib.import_module("aircombat-selfplay_amd.gru_train")


def _policy():
    return U.Policy(seed=3, device="cpu")


def _modules(pol):
    return list(pol.actor.modules()) + list(pol.critic.modules())


def test_use_device_mlp_finds_four_layers_and_keeps_everything(Mt):
    pol = _policy()
    params = [id(p) for p in list(pol.actor.parameters()) + list(pol.critic.parameters())]
    adam = [id(p) for grp in pol.optimizer.param_groups for p in grp["params"]]
    state = {k: v.clone() for m, pre in ((pol.actor, "a."), (pol.critic, "c.")) for k, v in ((pre + k, v) for k, v in m.state_dict().items())}
    fcs = [pol.actor.base.mlp.fc, pol.actor.act.mlp.fc, pol.critic.base.mlp.fc, pol.critic.mlp.fc]
    assert Mt.use_device_mlp(pol) == 4
    layers = [pol.actor.base.mlp, pol.actor.act.mlp, pol.critic.base.mlp, pol.critic.mlp]
    assert all(isinstance(m, Mt.DeviceMLPLayer) for m in layers)
    assert all(m.fc is fc for m, fc in zip(layers, fcs))                        # the very fc modules
    assert [id(p) for p in list(pol.actor.parameters()) + list(pol.critic.parameters())] == params == adam
    after = {k: v for m, pre in ((pol.actor, "a."), (pol.critic, "c.")) for k, v in ((pre + k, v) for k, v in m.state_dict().items())}
    assert list(after) == list(state) and all(torch.equal(after[k], state[k]) for k in state)
    assert "a.base.mlp.fc.0.weight" in after and "a.act.mlp.fc.5.bias" in after and "c.mlp.fc.3.weight" in after
    assert all(m.output_size == 128 for m in layers)
    assert Mt.use_device_mlp(pol) == 0                                           # already swapped
    assert Mt.use_device_mlp(pol.actor) == 0 and Mt.use_device_mlp(U.Actor()) == 2   # an nn.Module as the root


def test_composes_with_use_device_gru(Mt, Gt, monkeypatch):
    # use_device_gru refuses CPU parameters when it swaps; with that check lifted the composition is visible without a GPU
    monkeypatch.setattr(Gt, "check_gru", lambda gru, where="gru": None)
    for order in ("mlp first", "gru first"):
        pol = _policy()
        keys = list(pol.actor.state_dict()) + list(pol.critic.state_dict())
        params = [id(p) for p in list(pol.actor.parameters()) + list(pol.critic.parameters())]
        if order == "mlp first":
            assert Mt.use_device_mlp(pol) == 4 and Gt.use_device_gru(pol) == 2
        else:
            assert Gt.use_device_gru(pol) == 2 and Mt.use_device_mlp(pol) == 4
        assert sum(isinstance(m, Mt.DeviceMLPLayer) for m in _modules(pol)) == 4
        assert sum(isinstance(m, Gt.DeviceGRULayer) for m in _modules(pol)) == 2
        assert list(pol.actor.state_dict()) + list(pol.critic.state_dict()) == keys
        assert [id(p) for p in list(pol.actor.parameters()) + list(pol.critic.parameters())] == params


REFUSED = (
    ({"act": nn.Tanh()}, "activation Tanh"),
    ({"act": nn.LeakyReLU()}, "activation LeakyReLU"),
    ({"widths": (128, 64)}, "out-features 64"),
    ({"widths": (256, 128)}, "out-features 256"),
    ({"bias": False}, "without bias"),
    ({"affine": False}, "without affine"),
)


@pytest.mark.parametrize("kw,what", REFUSED, ids=[w for _, w in REFUSED])
def test_refusals_name_the_module_and_swap_nothing(Mt, pkg, kw, what):
    pol = _policy()
    pol.critic = U.Critic(**kw)          # the bad layer is found after the actor's two, which have passed their checks by then
    before = _modules(pol)
    with pytest.raises(pkg.UnsupportedPolicy, match=what) as e:
        Mt.use_device_mlp(pol)
    assert "critic.mlp.fc." in str(e.value)
    assert _modules(pol) == before and not any(isinstance(m, Mt.DeviceMLPLayer) for m in before)


def test_other_refusals(Mt, pkg):
    pol = _policy()
    pol.actor = U.Actor(obs=257)
    with pytest.raises(pkg.UnsupportedPolicy, match=r"actor\.base\.mlp\.fc\.0: in-features 257"):
        Mt.use_device_mlp(pol)
    assert not any(isinstance(m, Mt.DeviceMLPLayer) for m in _modules(pol))
    assert Mt.use_device_mlp(U.Actor(obs=256)) == 2                                 # 256 is in range
    pol = _policy()
    pol.critic.double()
    with pytest.raises(pkg.UnsupportedPolicy, match=r"critic\.mlp\.fc\.0: dtype torch.float64"):
        Mt.use_device_mlp(pol)
    assert not any(isinstance(m, Mt.DeviceMLPLayer) for m in _modules(pol))
    net = U.Base()
    net.mlp.fc[5] = nn.LayerNorm([1, 128])                                         # a LayerNorm over another shape
    with pytest.raises(pkg.UnsupportedPolicy, match=r"mlp\.fc\.3: LayerNorm over \(1, 128\)"):
        Mt.use_device_mlp(net)
    with pytest.raises(pkg.UnsupportedPolicy):
        Mt.use_device_mlp(object())
    with pytest.raises(pkg.UnsupportedPolicy, match="MLPLayer itself"):
        Mt.use_device_mlp(U.MLP(12))
    with pytest.raises(pkg.UnsupportedPolicy, match="activation_id 0"):
        Mt.DeviceMLPLayer(12, "128 128", 0)


def test_cpu_parameters_are_refused_at_call_time(Mt, pkg):
    net = U.Base()
    assert Mt.use_device_mlp(net) == 1          # swapping a CPU module is allowed: it can be moved afterwards
    with pytest.raises(pkg.UnsupportedPolicy, match=r"fc\.0: device cpu"):
        net(torch.zeros(4, U.OBS))


def test_device_mlp_layer_constructor(Mt):
    m = Mt.DeviceMLPLayer(15, "128 128", 1)
    assert list(m.state_dict()) == list(U.PNAMES) == list(U.MLP(15).state_dict())
    assert m.output_size == 128 and m.fc[0].in_features == 15 and m.fc[1] is m.fc[4]
    ref = U.MLP(21)
    assert Mt.DeviceMLPLayer(fc=ref.fc).fc is ref.fc


def test_exports(pkg):
    assert pkg.DeviceMLPLayer.__name__ == "DeviceMLPLayer" and callable(pkg.use_device_mlp) and callable(pkg.mlp_block)
    assert pkg.DeviceMLPBlockFunction
    assert all(n in pkg.__all__ for n in ("DeviceMLPBlockFunction", "DeviceMLPLayer", "mlp_block", "use_device_mlp"))


def test_capi_refusals(pkg):
    lib = pkg.load_library()
    assert all(hasattr(lib, n) for n in ("ac_mlp_block_workspace_floats", "ac_mlp_block_forward", "ac_mlp_block_backward"))
    p = 16   # never dereferenced: every call below is refused before it touches a device
    args_f = lambda M, K, null=-1: [0, None, M, K, 1e-5] + [None if i == null else p for i in range(6)] + [None]
    for null in range(6):   # x, w, b, gamma, beta, y (the seventh, stats, may be NULL)
        assert lib.ac_mlp_block_forward(*args_f(4, 8, null)) == -1
        assert "null argument" in lib.last_error()
    args_b = lambda M, K, null=-1: [0, None, M, K] + [None if i == null else p for i in range(7)] + [None] + [None if i + 8 == null else p for i in range(4)]
    for null in (0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11):   # dy, x, w, b, gamma, stats, workspace; dw, db, dgamma, dbeta (dx may be NULL)
        assert lib.ac_mlp_block_backward(*args_b(4, 8, null)) == -1
        assert "null argument" in lib.last_error()
    for M, K, what in ((0, 8, "M must be at least 1"), (-3, 8, "M must be at least 1"), (4, 0, "K must be 1 .. 256"), (4, 257, "K must be 1 .. 256"),
                       (1 << 24, 128, "32-bit index")):
        assert lib.ac_mlp_block_forward(*args_f(M, K)) == -1 and what in lib.last_error()
        assert lib.ac_mlp_block_backward(*args_b(M, K)) == -1 and what in lib.last_error()
        assert lib.ac_mlp_block_workspace_floats(M, K) == -1 and what in lib.last_error()
    # one set of 128 K + 384 partial sums per workgroup, one workgroup per 32-row tile up to 256
    assert lib.ac_mlp_block_workspace_floats(1, 12) == 128 * 12 + 384
    assert lib.ac_mlp_block_workspace_floats(33, 128) == 2 * (128 * 128 + 384)
    assert lib.ac_mlp_block_workspace_floats(4096 * 60, 256) == 256 * (128 * 256 + 384)
