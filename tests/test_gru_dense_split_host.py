"""The fused GRU layer's opt-in split-bf16 dense products (dense_products="bf16x3") without a GPU: a CPU emulation of the three products
with the six-term form held to the project's bound and the three-term form shown to miss it (tests/gru_dense_split_util.py), the
``dense_products`` argument of every Python entry that takes it, and the refusals of the ``_pd`` C entries."""
import importlib
import inspect

import pytest

import gru_dense_split_util as D
import gru_layer_util as LU

torch = pytest.importorskip("torch")
nn = torch.nn


@pytest.fixture(scope="module")
def G(pkg):
    return importlib.import_module("aircombat-selfplay_amd.gru_train")


@pytest.fixture(scope="module")
def L(pkg):
    return importlib.import_module("aircombat-selfplay_amd.gru_layer_train")


@pytest.mark.parametrize("seed", D.SEEDS)
@pytest.mark.parametrize("M", D.PRODUCT_ROWS)
@pytest.mark.parametrize("what", ["gi", "dx"])
def test_six_terms_meet_the_bound_and_three_miss_it(what, M, seed):
    e = D.errors(what, M, seed)
    print(f"emulation {what} M = {M} seed {seed}: fp32 {e['fp32']:.2e}, six terms {e['six']:.2e}, three terms {e['three']:.2e}, "
          f"bound {D.bound(e['fp32']):.2e}")
    assert e["six"] <= D.bound(e["fp32"]), (what, M, seed, e)
    assert e["three"] > D.bound(e["fp32"]), (what, M, seed, e)   # the bound tells the forms apart


@pytest.mark.parametrize("seed", D.SEEDS)
@pytest.mark.parametrize("rows", D.SHARE_ROWS)
def test_weight_gradient_share_meets_the_bound(rows, seed):
    """One workgroup's share of dW with a single fp32 accumulator for all six terms (the kernel's choice)."""
    e = D.errors("dW", rows, seed)
    print(f"emulation dW {rows} rows seed {seed}: fp32 {e['fp32']:.2e}, six terms {e['six']:.2e}, three terms {e['three']:.2e}, "
          f"bound {D.bound(e['fp32']):.2e}")
    assert e["six"] <= D.bound(e["fp32"]), (rows, seed, e)


def test_dense_products_argument_is_checked_everywhere(G, L, pkg):
    t = torch.zeros(1, 128)
    w, b = torch.zeros(384, 128), torch.zeros(384)
    net = nn.Module()
    net.rnn = LU.RefGRULayer()
    before = net.rnn
    for bad in ("fp16", "BF16X3", "", None, 1):
        if bad is not None:   # None there means "keep the layer's own"
            with pytest.raises(ValueError, match="dense_products"):
                L.use_device_gru_layer(net, dense_products=bad)
            with pytest.raises(ValueError, match="dense_products"):
                L.use_device_gru_layer(net, products="bf16x3", dense_products=bad)
        with pytest.raises(ValueError, match="dense_products"):
            L.gru_layer(t, t, torch.ones(1), w, w, b, b, torch.ones(128), torch.zeros(128), dense_products=bad)
        with pytest.raises(ValueError, match="dense_products"):
            L.DeviceFusedGRULayer(dense_products=bad)
        with pytest.raises(ValueError, match="dense_products"):
            L.DeviceFusedGRULayer(products="bf16x3", dense_products=bad)
        assert net.rnn is before   # refused before a module is touched
    with pytest.raises(ValueError, match="dense_products"):   # even an object that is no policy at all is not looked at first
        L.use_device_gru_layer(object(), dense_products="fp16")
    assert L.DeviceFusedGRULayer().dense_products == "fp32" and L.DeviceFusedGRULayer(products="bf16x3").dense_products == "fp32"
    both = L.DeviceFusedGRULayer(products="bf16x3", dense_products="bf16x3")
    assert (both.products, both.dense_products) == ("bf16x3", "bf16x3")
    only = L.DeviceFusedGRULayer(dense_products="bf16x3")
    assert (only.products, only.dense_products) == ("fp32", "bf16x3")   # the two selectors are independent
    # their dense products are torch's: no such argument
    assert "dense_products" not in inspect.signature(G.DeviceGRULayer.__init__).parameters
    assert "dense_products" not in inspect.signature(G.use_device_gru).parameters
    assert inspect.signature(L.gru_layer).parameters["dense_products"].default == "fp32"
    assert inspect.signature(L.use_device_gru_layer).parameters["dense_products"].default is None


def _policy():
    policy = type("PPOPolicy", (), {})()
    policy.actor, policy.critic = nn.Module(), nn.Module()
    policy.actor.rnn, policy.critic.rnn = LU.RefGRULayer(), LU.RefGRULayer()
    return policy


def test_swaps_carry_dense_products(G, L, monkeypatch):
    monkeypatch.setattr(G, "check_gru", lambda gru, where="gru": None)
    monkeypatch.setattr(L, "check_layer", lambda gru, norm, where="rnn": None)
    pol = _policy()
    gru = pol.actor.rnn.gru
    assert L.use_device_gru_layer(pol, dense_products="bf16x3") == 2
    for rnn in (pol.actor.rnn, pol.critic.rnn):
        assert type(rnn) is L.DeviceFusedGRULayer and (rnn.products, rnn.dense_products) == ("fp32", "bf16x3")
    assert pol.actor.rnn.gru is gru
    kept = pol.actor.rnn
    assert L.use_device_gru_layer(pol) == 0 and pol.actor.rnn is kept and kept.dense_products == "bf16x3"   # a fused layer keeps its own
    pol = _policy()
    assert G.use_device_gru(pol, products="bf16x3") == 2   # a DeviceGRULayer: its products kept, dense_products as given or the default
    assert L.use_device_gru_layer(pol, dense_products="bf16x3") == 2
    assert (pol.critic.rnn.products, pol.critic.rnn.dense_products) == ("bf16x3", "bf16x3")
    pol = _policy()
    assert G.use_device_gru(pol, products="bf16x3") == 2 and L.use_device_gru_layer(pol) == 2
    assert (pol.actor.rnn.products, pol.actor.rnn.dense_products) == ("bf16x3", "fp32")
    pol = _policy()
    assert L.use_device_gru_layer(pol, products="bf16x3", dense_products="fp32") == 2
    assert (pol.actor.rnn.products, pol.actor.rnn.dense_products) == ("bf16x3", "fp32")
    pol = _policy()
    assert L.use_device_gru_layer(pol) == 2 and pol.actor.rnn.dense_products == "fp32"   # a plain GRULayer: the default


SYMS = ("ac_gru_layer_forward_pd", "ac_gru_layer_backward_pd")


def test_symbols(pkg):
    lib = pkg.load_library()
    for sym in SYMS:
        assert sym in pkg.capi.SIGNATURES and hasattr(lib, sym)
        old, new = pkg.capi.SIGNATURES[sym[:-1]], pkg.capi.SIGNATURES[sym]
        assert new[0] is old[0] and new[1][:-1] == old[1] and new[1][-1] is old[1][-1]   # the `_p` list plus one int32


def _args(sym, N=4, T=8, null=-1, products=1, dense=1):
    p = 16   # never dereferenced: every call made with these is refused before it touches a device
    ptr = lambda i: None if i == null else p
    if sym == "ac_gru_layer_forward_pd":
        body = [ptr(i) for i in range(9)] + [1e-5] + [ptr(9 + i) for i in range(4)] + [p, p]
    else:
        body = [None, None] + [ptr(i) for i in range(10)] + [None, None] + [ptr(10 + i) for i in range(6)]
    return [0, None, N, T] + body + [products, dense]


REQUIRED = {"ac_gru_layer_forward_pd": 13, "ac_gru_layer_backward_pd": 16}


@pytest.mark.parametrize("sym", SYMS)
def test_capi_refusals(pkg, sym):
    lib = pkg.load_library()
    fn = getattr(lib, sym)
    said = set()
    for products in (0, 1):
        for dense in (0, 1):
            for null in range(REQUIRED[sym]):
                assert fn(*_args(sym, null=null, products=products, dense=dense)) == -1
                assert "null argument" in lib.last_error() and sym + ":" in lib.last_error()
            said.add(lib.last_error())
            for N, T in ((0, 8), (4, 0), (-1, 2)):
                assert fn(*_args(sym, N, T, products=products, dense=dense)) == -1
                assert "at least 1" in lib.last_error() and sym + ":" in lib.last_error()
            said.add(lib.last_error())
            assert fn(*_args(sym, 1 << 16, 1 << 15, products=products, dense=dense)) == -1
            assert "32-bit row index" in lib.last_error() and sym + ":" in lib.last_error()
            said.add(lib.last_error())
            args = _args(sym, products=products, dense=dense)
            args[4 if sym == SYMS[0] else 6] = 20   # x off its 16 bytes
            assert fn(*args) == -1 and "16-byte aligned" in lib.last_error() and sym + ":" in lib.last_error()
            said.add(lib.last_error())
    if sym == SYMS[0]:   # saved without stats
        args = _args(sym)
        args[-3] = None
        assert fn(*args) == -1 and "saved and stats go together" in lib.last_error() and sym + ":" in lib.last_error()
    for dense in (0, 1):
        for products in (2, -1, 7):
            assert fn(*_args(sym, products=products, dense=dense)) == -1
            assert "unknown products" in lib.last_error() and sym + ":" in lib.last_error() and str(products) in lib.last_error()
    said.add(lib.last_error())
    for products in (0, 1):
        for dense in (2, -1, 7):
            assert fn(*_args(sym, products=products, dense=dense)) == -1
            assert "unknown dense products" in lib.last_error() and sym + ":" in lib.last_error() and str(dense) in lib.last_error()
    said.add(lib.last_error())
    assert len(said) == 6   # six refusals, six messages
