"""The training GRU's opt-in split-bf16 product (products="bf16x3") without a GPU: a CPU emulation of the forward recurrence with the
six-term product held to the project's bound and the three-term product shown to miss it (tests/gru_split_util.py), the ``products``
argument of every Python entry, and the refusals of the ``_p`` C entries."""
import importlib

import numpy as np
import pytest

import gru_layer_util as LU
import gru_split_util as S
import gru_train_util as GU

torch = pytest.importorskip("torch")
nn = torch.nn


@pytest.fixture(scope="module")
def G(pkg):
    return importlib.import_module("aircombat-selfplay_amd.gru_train")


@pytest.fixture(scope="module")
def L(pkg):
    return importlib.import_module("aircombat-selfplay_amd.gru_layer_train")


def test_pieces_add_up_exactly():
    x = np.concatenate([GU.inputs("mix")["weight_hh_l0"].ravel(), GU.inputs("mix")["hxs"].ravel(), np.float32([0.0, -0.0, 1.0, -3.0])])
    b0, b1, b2 = S.split3(x)
    for b in (b0, b1, b2):
        assert not (b.view(np.uint32) & 0xFFFF).any()   # each piece is a bf16
    assert np.array_equal((b0.astype(np.float64) + b1) + b2, x.astype(np.float64))
    z = S.split3(np.float32([0.0, -0.0]))
    assert all(not p.any() for p in z)   # a masked value splits to three zero pieces


_runs = {}
SCALED = 4.0   # W_hh times this in the runs that tell the three-term form from the six-term one


def _case(name, scale=1.0):
    """The four forms of the recurrence on a case, computed once: float64, torch fp32, six terms, three terms."""
    if (name, scale) not in _runs:
        N, T, _ = GU.CASES[name]
        inp = GU.inputs(name)
        inp["weight_hh_l0"] = inp["weight_hh_l0"] * np.float32(scale)
        _runs[name, scale] = {form: S.recurrence(inp, N, T, form) for form in ("f64", "fp32", "six", "three")}
    return _runs[name, scale]


@pytest.mark.parametrize("name", list(GU.CASES))
def test_float64_recurrence_is_the_golden_layer(name):
    y, h_T = _case(name)["f64"]
    g = GU.golden()
    assert S.rel(S.layer_norm64(y), g[f"{name}/out"]) < 1e-6 and S.rel(h_T, g[f"{name}/h_T"]) < 1e-6   # the fixture is stored as float32


@pytest.mark.parametrize("name", list(GU.CASES))
def test_six_terms_meet_the_bound_and_three_miss_it(name):
    """With the cases' own W_hh (uniform in +- 1/sqrt(128)) the three-term form misses the bound on y by a factor of 1.1 (mix) to 2.0
    (t1) only, measured here; a margin that thin could turn with another BLAS behind torch's fp32 matmul. So the two forms are told
    apart with W_hh scaled by 4 (the hidden product's share of the gates grows, the bound stays the same formula): there the
    three-term form misses by 4 to 11 times, and the six-term form must meet the bound at both scales."""
    for scale in (1.0, SCALED):
        runs = _case(name, scale)
        for i, what in enumerate(("y", "h_T")):
            ref = runs["f64"][i]
            e_ref, e_six, e_three = (S.rel(runs[form][i], ref) for form in ("fp32", "six", "three"))
            print(f"emulation {name} W_hh x {scale:g} {what}: fp32 {e_ref:.2e}, six terms {e_six:.2e}, three terms {e_three:.2e}, "
                  f"bound {S.bound(e_ref):.2e}")
            assert e_six <= S.bound(e_ref), (name, scale, what, e_six, e_ref)
            if scale == SCALED and what == "y":
                assert e_three > S.bound(e_ref), (name, what, e_three, e_ref)


def test_products_argument_is_checked_everywhere(G, L, pkg):
    t = torch.zeros(1, 128)
    w, b = torch.zeros(384, 128), torch.zeros(384)
    net = nn.Module()
    net.rnn = LU.RefGRULayer()
    before = net.rnn
    for bad in ("fp16", "BF16X3", "", None, 1):
        with pytest.raises(ValueError, match="products"):
            G.gru_seq(t, t, torch.ones(1), w, w, b, b, products=bad)
        with pytest.raises(ValueError, match="products"):
            G.DeviceGRULayer(products=bad)
        with pytest.raises(ValueError, match="products"):
            L.DeviceFusedGRULayer(products=bad)
        with pytest.raises(ValueError, match="products"):
            G.use_device_gru(net, products=bad)
        if bad is not None:   # None there means "keep the layer's own"
            with pytest.raises(ValueError, match="products"):
                L.gru_layer(t, t, torch.ones(1), w, w, b, b, torch.ones(128), torch.zeros(128), products=bad)
            with pytest.raises(ValueError, match="products"):
                L.use_device_gru_layer(net, products=bad)
        assert net.rnn is before   # refused before a module is touched
    # even an object that is no policy at all is not looked at first
    with pytest.raises(ValueError, match="products"):
        G.use_device_gru(object(), products="fp16")
    with pytest.raises(ValueError, match="products"):
        L.use_device_gru_layer(object(), products="fp16")
    assert G.DeviceGRULayer().products == "fp32" and L.DeviceFusedGRULayer().products == "fp32"
    assert G.DeviceGRULayer(products="bf16x3").products == "bf16x3" and L.DeviceFusedGRULayer(products="bf16x3").products == "bf16x3"
    assert pkg.DeviceGRULayer is G.DeviceGRULayer


def _policy():
    policy = type("PPOPolicy", (), {})()
    policy.actor, policy.critic = nn.Module(), nn.Module()
    policy.actor.rnn, policy.critic.rnn = LU.RefGRULayer(), LU.RefGRULayer()
    return policy


def test_swaps_carry_products(G, L, monkeypatch):
    monkeypatch.setattr(G, "check_gru", lambda gru, where="gru": None)
    monkeypatch.setattr(L, "check_layer", lambda gru, norm, where="rnn": None)
    pol = _policy()
    gru = pol.actor.rnn.gru
    assert G.use_device_gru(pol, products="bf16x3") == 2
    assert type(pol.actor.rnn) is G.DeviceGRULayer and pol.actor.rnn.products == pol.critic.rnn.products == "bf16x3"
    assert L.use_device_gru_layer(pol) == 2   # keeps each layer's own
    assert type(pol.actor.rnn) is L.DeviceFusedGRULayer and pol.actor.rnn.products == pol.critic.rnn.products == "bf16x3"
    assert pol.actor.rnn.gru is gru
    pol = _policy()
    assert G.use_device_gru(pol, products="bf16x3") == 2 and L.use_device_gru_layer(pol, products="fp32") == 2   # unless given one
    assert pol.actor.rnn.products == "fp32"
    pol = _policy()
    assert G.use_device_gru(pol) == 2 and pol.actor.rnn.products == "fp32"
    assert L.use_device_gru_layer(pol, products="bf16x3") == 2 and pol.critic.rnn.products == "bf16x3"
    pol = _policy()
    assert L.use_device_gru_layer(pol) == 2 and pol.actor.rnn.products == "fp32"   # a plain GRULayer: the default


SYMS = ("ac_gru_seq_forward_p", "ac_gru_seq_backward_p", "ac_gru_layer_forward_p", "ac_gru_layer_backward_p")


def test_symbols_and_constants(pkg, G):
    lib = pkg.load_library()
    for sym in SYMS:
        assert sym in pkg.capi.SIGNATURES and hasattr(lib, sym)
        old = pkg.capi.SIGNATURES[sym[:-2]]
        assert pkg.capi.SIGNATURES[sym][0] is old[0] and len(pkg.capi.SIGNATURES[sym][1]) == len(old[1]) + 1   # the old list plus products
    assert G.PRODUCTS == {"fp32": 0, "bf16x3": 1}


def _args(sym, N=4, T=8, null=-1, products=1):
    p = 16   # never dereferenced: every call made with these is refused before it touches a device
    ptr = lambda i: None if i == null else p
    if sym == "ac_gru_seq_forward_p":
        body = [ptr(i) for i in range(8)]
    elif sym == "ac_gru_seq_backward_p":
        body = [None, None] + [ptr(i) for i in range(7)] + [None]
    elif sym == "ac_gru_layer_forward_p":
        body = [ptr(i) for i in range(9)] + [1e-5] + [ptr(9 + i) for i in range(4)] + [p, p]
    else:
        body = [None, None] + [ptr(i) for i in range(10)] + [None, None] + [ptr(10 + i) for i in range(6)]
    return [0, None, N, T] + body + [products]


REQUIRED = {"ac_gru_seq_forward_p": 7, "ac_gru_seq_backward_p": 7, "ac_gru_layer_forward_p": 13, "ac_gru_layer_backward_p": 16}


@pytest.mark.parametrize("sym", SYMS)
def test_capi_refusals(pkg, sym):
    lib = pkg.load_library()
    fn = getattr(lib, sym)
    said = set()
    for products in (0, 1):
        for null in range(REQUIRED[sym]):
            assert fn(*_args(sym, null=null, products=products)) == -1
            assert "null argument" in lib.last_error() and sym in lib.last_error()
        said.add(lib.last_error())
        for N, T in ((0, 8), (4, 0), (-1, 2)):
            assert fn(*_args(sym, N, T, products=products)) == -1
            assert "at least 1" in lib.last_error() and sym in lib.last_error()
        said.add(lib.last_error())
        assert fn(*_args(sym, 1 << 16, 1 << 15, products=products)) == -1 and "32-bit row index" in lib.last_error()
    for products in (2, -1, 7):
        assert fn(*_args(sym, products=products)) == -1
        assert "unknown products" in lib.last_error() and sym in lib.last_error() and str(products) in lib.last_error()
    said.add(lib.last_error())
    assert len(said) == 3   # three refusals, three messages
