"""The training MLP blocks' opt-in split-bf16 products (products="bf16x3": csrc/mlp_train_split.hpp) without a GPU: a CPU emulation of
a two-block layer with the six-term products held to the project's bound and the three-term form shown to miss it
(tests/mlp_split_util.py), the condition on the golden inputs that keeps the ReLU mask out of the comparison, the ``products`` argument
of every Python entry that takes it, and the new C entries' table rows, constants and refusals."""
import importlib
import inspect

import numpy as np
import pytest

import mlp_split_util as S
import mlp_train_util as U

torch = pytest.importorskip("torch")
nn = torch.nn


@pytest.fixture(scope="module")
def Mt(pkg):
    return importlib.import_module("aircombat-selfplay_amd.mlp_train")


# ---- 1. the emulation of a two-block layer
@pytest.mark.parametrize("name", list(U.CASES))
def test_six_terms_meet_the_bound_and_three_miss_it(name):
    f64, fp32, six, three = (S.emulated(name, form)[0] for form in ("f64", "fp32", "six", "three"))
    assert set(six) == set(U.keys(name))
    for k in U.keys(name):
        e_ref, e_six, e_three = S.rel(fp32[k], f64[k]), S.rel(six[k], f64[k]), S.rel(three[k], f64[k])
        print(f"emulation {name} {k}: fp32 {e_ref:.2e}, six terms {e_six:.2e}, three terms {e_three:.2e}, bound {S.bound(e_ref):.2e}")
        assert e_six <= S.bound(e_ref), (name, k, e_six, e_ref)
        if k in ("y0", "y1"):
            assert e_three > S.bound(e_ref), (name, k, e_three, e_ref)   # the bound tells the forms apart


# ---- 2. no pre-activation of the golden cases sits where the forms could disagree about the ReLU mask
@pytest.mark.parametrize("name", list(U.CASES))
def test_no_pre_activation_near_zero(name):
    z64 = S.emulated(name, "f64")[1]
    for blk in (0, 1):
        err = max(float(np.abs(S.emulated(name, form)[1][blk] - z64[blk]).max()) for form in ("fp32", "six"))
        nz = np.abs(z64[blk][z64[blk] != 0.0])
        print(f"{name} block {blk}: smallest non-zero |z64| {nz.min():.2e}, largest z error {err:.2e}")
        assert nz.min() >= 8 * err, (name, blk, float(nz.min()), err)
        for form in ("fp32", "six"):   # and so the masks agree (an exact 0 in float64 is an exact 0 in either form: x = 0, b = 0)
            assert np.array_equal(S.emulated(name, form)[1][blk] > 0, z64[blk] > 0)


# ---- 3. the argument
def _net():
    net = nn.Module()
    net.base, net.head = U.Base(15), U.MLP(128)
    return net


def test_products_argument_is_checked_everywhere(Mt):
    x, lin, norm = torch.zeros(2, 15), nn.Linear(15, 128), nn.LayerNorm(128)
    net = _net()
    before = (net.base.mlp, net.head)
    for bad in ("fp16", "BF16X3", "", None, 1):
        with pytest.raises(ValueError, match="products"):
            Mt.mlp_block(x, lin, norm, products=bad)
        with pytest.raises(ValueError, match="products"):
            Mt.DeviceMLPLayer(products=bad)
        with pytest.raises(ValueError, match="products"):
            Mt.DeviceMLPLayer(fc=net.head.fc, products=bad)
        with pytest.raises(ValueError, match="products"):
            Mt.use_device_mlp(net, products=bad)
        assert (net.base.mlp, net.head) == before and not any(isinstance(m, Mt.DeviceMLPLayer) for m in net.modules())
    with pytest.raises(ValueError, match="products"):   # even an object that is no policy at all is not looked at first
        Mt.use_device_mlp(object(), products="fp16")
    for fn in (Mt.mlp_block, Mt.DeviceMLPLayer.__init__, Mt.use_device_mlp):
        assert inspect.signature(fn).parameters["products"].default == "fp32"
    assert Mt.DeviceMLPLayer().products == "fp32" and Mt.DeviceMLPLayer(15, products="bf16x3").products == "bf16x3"


def test_swaps_carry_products(Mt):
    net = _net()
    fcs = (net.base.mlp.fc, net.head.fc)
    assert Mt.use_device_mlp(net, products="bf16x3") == 2
    for layer, fc in zip((net.base.mlp, net.head), fcs):
        assert type(layer) is Mt.DeviceMLPLayer and layer.products == "bf16x3" and layer.fc is fc
    kept = net.head
    assert Mt.use_device_mlp(net) == 0 and net.head is kept and kept.products == "bf16x3"   # a device layer keeps its own
    net = _net()
    assert Mt.use_device_mlp(net) == 2 and net.base.mlp.products == net.head.products == "fp32"   # the default
    assert "products" not in net.head.state_dict() and list(net.head.state_dict()) == list(U.MLP(128).state_dict())


def test_layer_gives_its_products_to_every_block(Mt, monkeypatch):
    seen = []
    monkeypatch.setattr(Mt, "mlp_block", lambda x, lin, norm, where, products: (seen.append(products), x.new_zeros(x.shape[:-1] + (128,)))[1])
    for products in S.PRODUCTS:
        Mt.DeviceMLPLayer(15, products=products)(torch.zeros(3, 15))
    assert seen == ["fp32", "fp32", "bf16x3", "bf16x3"]


# ---- the C entries
SYMS = ("ac_mlp_block_forward_p", "ac_mlp_block_backward_p")


def test_symbols_and_constants(pkg):
    lib = pkg.load_library()
    for sym in SYMS:
        assert sym in pkg.capi.SIGNATURES and hasattr(lib, sym)
        old, new = pkg.capi.SIGNATURES[sym[:-2]], pkg.capi.SIGNATURES[sym]
        assert new[0] is old[0] and new[1][:-1] == old[1] and new[1][-1] is old[1][2]   # the old list plus one int32
    assert [lib.ac_mlp_block_constant(i) for i in (0, 1, 2)] == [32, 512, 256]
    mask = lib.ac_mlp_block_constant(3)
    assert mask & ~S.KP_ALL == 0 and lib.ac_mlp_block_constant(4) == -1 and lib.ac_mlp_block_constant(-1) == -1


def _args(sym, M=8, K=12, null=-1, products=1):
    p = 16   # never dereferenced: every call made with these is refused before it touches a device
    ptr = lambda i: None if i == null else p
    if sym == SYMS[0]:
        return [0, None, M, K, 1e-5] + [ptr(i) for i in range(6)] + [p, products]
    return [0, None, M, K] + [ptr(i) for i in range(7)] + [p] + [ptr(7 + i) for i in range(4)] + [products]


REQUIRED = {SYMS[0]: 6, SYMS[1]: 11}


@pytest.mark.parametrize("sym", SYMS)
def test_capi_refusals(pkg, sym):
    lib = pkg.load_library()
    fn = getattr(lib, sym)
    for products in (2, -1, 7):
        assert fn(*_args(sym, products=products)) == -1
        assert "unknown products" in lib.last_error() and sym + ":" in lib.last_error() and str(products) in lib.last_error()
    for products in (0, 1):
        for null in range(REQUIRED[sym]):
            assert fn(*_args(sym, null=null, products=products)) == -1
            assert "null argument" in lib.last_error() and sym + ":" in lib.last_error(), (null, lib.last_error())
        for M, K, what in ((8, 0, "K must be"), (8, 257, "K must be"), (0, 12, "M must be")):
            assert fn(*_args(sym, M, K, products=products)) == -1
            assert what in lib.last_error() and sym + ":" in lib.last_error()
