"""The training GRU without a GPU: the tests' float64 restatement of the reference's GRULayer against tests/golden/gru_train.npz, the
refusals of use_device_gru and its parameter-identity rule on CPU modules, and the C ABI refusals that return before touching a device."""
import importlib

import numpy as np
import pytest

import gru_train_util as U

torch = pytest.importorskip("torch")
nn = torch.nn


def _f64_case(name):
    inp = U.inputs(name)
    p = {k: torch.tensor(inp[k], dtype=torch.float64, requires_grad=True) for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")}
    t = lambda k, g=False: torch.tensor(inp[k], dtype=torch.float64, requires_grad=g)
    N, T, _ = U.CASES[name]
    return U.run_with_grads(lambda x, h, m: U.step_layer(p, x, h, m, N, T), p, t("x", True), t("hxs", True), t("masks"), t("g_out"), t("g_h"))


@pytest.mark.parametrize("name", list(U.CASES))
def test_float64_restatement_matches_golden(name):
    g = U.golden()
    res = _f64_case(name)
    for k in U.KEYS:
        s = U.stored(k, res[k])
        ref = g[f"{name}/{k}"]
        assert s.shape == ref.shape, (k, s.shape, ref.shape)
        # the float64 projection to 1e-12, every element to the float32 storage's rounding
        p, rp = U.project(k, s), float(g[f"{name}/{k}@p"])
        scale = float(np.abs(s.ravel()) @ np.abs(U.projector(k, s.size)))
        assert abs(p - rp) <= 1e-12 * scale, (name, k, p, rp)
        assert np.abs(s - ref).max() <= 2.0 ** -23 * np.abs(s).max() + 1e-30, (name, k)


def test_cases_cover_the_mask_patterns():
    m = {n: U.masks(n).reshape(U.CASES[n][1], U.CASES[n][0]) for n in U.CASES}
    mix = m["mix"]
    assert (mix[0] == 0).any() and (mix[0] == 1).any()           # zero at t = 0 for some rows
    assert (mix[1:] == 0).any(axis=1).sum() >= 2                 # zeros mid-chunk
    assert (mix == 0).all(axis=1).any()                          # a step where every row's mask is 0
    assert (m["long"] == 1).all() and U.CASES["long"][1] == 60    # no zeros, T = 60
    assert U.CASES["single"][0] == 1 and U.CASES["t1"][1] == 1 and U.CASES["mix"][0] % 16 and U.CASES["mix"][1] == 8


@pytest.fixture(scope="module")
def G(pkg):
    return importlib.import_module("aircombat-selfplay_amd.gru_train")


class _Layer(nn.Module):   # the reference's GRULayer children, CPU
    def __init__(self, i=128, h=128, layers=1, **kw):
        super().__init__()
        self._num_layers = layers
        self.gru = nn.GRU(input_size=i, hidden_size=h, num_layers=layers, **kw)
        self.norm = nn.LayerNorm(h)


class _Net(nn.Module):
    def __init__(self, **kw):
        super().__init__()
        self.base = nn.Linear(4, 128)
        self.rnn = _Layer(**kw)


def test_use_device_gru_refuses_cpu_and_other_shapes(G, pkg):
    for kw, what in (({}, "device"), ({"h": 64}, "sizes"), ({"layers": 2}, "layers"), ({"bias": False}, "no bias"),
                     ({"batch_first": True}, "batch_first")):
        net = _Net(**kw)
        before = net.rnn
        with pytest.raises(pkg.UnsupportedPolicy, match=what):
            G.use_device_gru(net)
        assert net.rnn is before   # nothing swapped when refused
    net = _Net().double()
    with pytest.raises(pkg.UnsupportedPolicy, match="float32"):
        G.use_device_gru(net)
    with pytest.raises(pkg.UnsupportedPolicy, match="rnn.gru"):   # refusals name the layer
        G.use_device_gru(_Net())
    with pytest.raises(pkg.UnsupportedPolicy):
        G.use_device_gru(object())
    with pytest.raises(pkg.UnsupportedPolicy, match="GRULayer itself"):
        G.use_device_gru(_Layer())


def test_swapped_layer_keeps_parameters_and_state_dict(G, monkeypatch):
    # the device check is what refuses a CPU module; with it lifted the swap itself is visible on the CPU
    monkeypatch.setattr(G, "check_gru", lambda gru, where="gru": None)
    actor, critic = _Net(), _Net()
    policy = type("PPOPolicy", (), {})()
    policy.actor, policy.critic = actor, critic
    params = {id(p) for p in list(actor.parameters()) + list(critic.parameters())}
    keys = list(actor.state_dict()) + list(critic.state_dict())
    gru, norm = actor.rnn.gru, actor.rnn.norm
    assert G.use_device_gru(policy) == 2
    assert isinstance(actor.rnn, G.DeviceGRULayer) and isinstance(critic.rnn, G.DeviceGRULayer)
    assert actor.rnn.gru is gru and actor.rnn.norm is norm
    assert {id(p) for p in list(actor.parameters()) + list(critic.parameters())} == params
    assert list(actor.state_dict()) + list(critic.state_dict()) == keys
    assert G.use_device_gru(policy) == 0    # already swapped
    assert actor.rnn.output_size == 128


def test_exports(pkg):
    assert pkg.DeviceGRULayer.__name__ == "DeviceGRULayer" and callable(pkg.use_device_gru) and pkg.DeviceGRUFunction


def test_capi_refusals(pkg):
    lib = pkg.load_library()
    p = 16   # never dereferenced: every call below is refused before it touches a device
    args_f = lambda N, T, null=-1: [0, None, N, T] + [None if i == null else p for i in range(8)]
    for null in range(7):   # every required pointer of the forward (the eighth, saved, may be NULL)
        assert lib.ac_gru_seq_forward(*args_f(4, 8, null)) == -1
        assert "null argument" in lib.last_error()
    for N, T in ((0, 8), (4, 0), (-1, 2)):
        assert lib.ac_gru_seq_forward(*args_f(N, T)) == -1
        assert "at least 1" in lib.last_error()
    assert lib.ac_gru_seq_forward(*args_f(1 << 16, 1 << 15)) == -1
    assert "32-bit row index" in lib.last_error()
    args_b = lambda N, T, null=-1: [0, None, N, T, None, None] + [None if i == null else p for i in range(7)] + [None]
    for null in range(7):   # saved, y, hxs, masks, w_hh, dgi, dgh
        assert lib.ac_gru_seq_backward(*args_b(4, 8, null)) == -1
        assert "null argument" in lib.last_error()
    for N, T in ((0, 8), (4, 0)):
        assert lib.ac_gru_seq_backward(*args_b(N, T)) == -1
        assert "at least 1" in lib.last_error()
    assert lib.ac_gru_seq_backward(*args_b(1 << 20, 1 << 12)) == -1
    assert "32-bit row index" in lib.last_error()
