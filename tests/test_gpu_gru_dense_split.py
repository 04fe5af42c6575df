"""The fused GRU layer's opt-in split-bf16 dense products (dense_products="bf16x3": csrc/gru_layer_train_split.hpp) on the MI355X,
through DeviceFusedGRULayer under both ``products``: against the reference's float64 GRULayer (tests/golden/gru_train.npz), against
the tests' float64 restatement at the tile edges in M = N T and over 60 steps with several tiles per workgroup, without a gradient
for x or hxs, the untouched default, determinism, stream discipline, all-zero and all-one masks and a whole PPO update.

The bound everywhere is gru_split_util's: with rel(a, ref) = max|a - ref| / max|ref| against float64, rel(device) <=
max(4 * rel(torch fp32), 2^-20), where torch fp32 is the reference-form layer on the same GPU and inputs."""
import copy
import importlib

import numpy as np
import pytest

import gru_layer_util as U
import gru_train_util as GU
from gru_split_util import bound, rel

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
nn = torch.nn
PRODUCTS = ("fp32", "bf16x3")


@pytest.fixture(scope="module")
def L(pkg):
    return importlib.import_module("aircombat-selfplay_amd.gru_layer_train")


def device_layer(L, inp, products, dense="bf16x3"):
    holder = nn.Module()
    holder.rnn = U.layer_from(inp)
    assert L.use_device_gru_layer(holder, products=products, dense_products=dense) == 1 and type(holder.rnn) is L.DeviceFusedGRULayer
    assert (holder.rnn.products, holder.rnn.dense_products) == (products, dense)
    return holder.rnn


def run(layer, inp, over=None, x_grad=True, h_grad=True):
    src = dict(inp, **(over or {}))
    c = lambda k, g=False: torch.tensor(src[k], dtype=torch.float32, device="cuda", requires_grad=g)
    params = U.layer_params(layer)
    for p in params.values():
        p.grad = None
    if x_grad and h_grad:
        return U.run_with_grads(layer, params, c("x", True), c("hxs", True), c("masks"), c("g_out"), c("g_h"))
    x, hxs = c("x", x_grad), c("hxs", h_grad)
    out, h_T = layer(x, hxs, c("masks"))
    ((out * c("g_out")).sum() + (h_T * c("g_h")).sum()).backward()
    res = {"out": out, "h_T": h_T, "dgamma": params["norm.weight"].grad, "dbeta": params["norm.bias"].grad}
    res.update({"d" + k[:-3].replace("weight", "W").replace("bias", "b"): params[k].grad for k in U.GRU_NAMES})
    if x_grad:
        res["dx"] = x.grad
    if h_grad:
        res["dhxs"] = hxs.grad
    return {k: v.detach().double().cpu().numpy().reshape(-1, U.H) if k in ("h_T", "dhxs") else v.detach().double().cpu().numpy() for k, v in res.items()}


def run_f64(inp, N, T):
    names = U.GRU_NAMES + tuple(k for k in U.NORM_NAMES if k in inp)
    p = {k: torch.tensor(inp[k], dtype=torch.float64, device="cuda", requires_grad=True) for k in names}
    c = lambda k, g=False: torch.tensor(inp[k], dtype=torch.float64, device="cuda", requires_grad=g)
    return U.run_with_grads(lambda x, h, m: U.step_layer(p, x, h, m, N, T), p, c("x", True), c("hxs", True), c("masks"), c("g_out"), c("g_h"))


_f64, _ref = {}, {}


def refs(tag, inp, N, T):
    """(float64, torch fp32 in the reference's form) of a case, computed once."""
    if tag not in _f64:
        _f64[tag], _ref[tag] = run_f64(inp, N, T), run(U.layer_from(inp), inp)
    return _f64[tag], _ref[tag]


def held(what, products, split, ref, f64, keys=U.KEYS, pick=lambda k, a: a):
    for k in keys:
        assert np.isfinite(split[k]).all(), (what, k)
        e_dev, e_ref = rel(pick(k, split[k]), f64[k]), rel(pick(k, ref[k]), f64[k])
        print(f"{what} products={products} {k}: dense bf16x3 {e_dev:.2e}, torch fp32 {e_ref:.2e}, bound {bound(e_ref):.2e}")
        assert e_dev <= bound(e_ref), (what, products, k, e_dev, e_ref)


# ---- 1. the golden cases
@pytest.mark.parametrize("products", PRODUCTS)
@pytest.mark.parametrize("name", list(GU.CASES))
def test_golden_agreement(L, name, products):
    g, inp = GU.golden(), GU.inputs(name)   # no norm.weight / norm.bias: the LayerNorm keeps its unit scale and zero shift
    gold = {k: g[f"{name}/{k}"] for k in GU.KEYS}
    held(f"golden {name}", products, run(device_layer(L, inp, products), inp), run(U.layer_from(inp), inp), gold, keys=GU.KEYS, pick=GU.stored)


# ---- 2. the tile edges in M = N T: 31, 32, 33, 65, 64, 51 rows
@pytest.mark.parametrize("products", PRODUCTS)
@pytest.mark.parametrize("N,T", [(31, 1), (32, 1), (33, 1), (13, 5), (16, 4), (17, 3)])
def test_tile_edges(L, N, T, products):
    inp = U.edge_inputs(N, T)
    f64, ref = refs((N, T), inp, N, T)
    held(f"edge {N} x {T}", products, run(device_layer(L, inp, products), inp), ref, f64)


# ---- 3. sixty steps: 510 tiles, two per workgroup of gi / dx and four per workgroup of dw
def _long():
    N, T = 272, 60
    inp = U.random_inputs(N, T, done=0.02)
    assert (inp["masks"] == 0).any()
    return N, T, inp


@pytest.mark.parametrize("products", PRODUCTS)
def test_several_tiles_per_workgroup(L, pkg, products):
    N, T, inp = _long()
    lib = pkg.load_library()
    tiles = -(-N * T // lib.ac_gru_layer_constant(0))
    assert tiles == 510 and tiles > lib.ac_gru_layer_constant(1) and tiles > lib.ac_gru_layer_constant(5) and tiles > 3 * lib.ac_gru_layer_constant(4)
    f64, ref = refs("long", inp, N, T)
    split = run(device_layer(L, inp, products), inp)
    held(f"long {N} x {T}", products, split, ref, f64)
    exact = run(device_layer(L, inp, products, "fp32"), inp)
    assert any(not np.array_equal(split[k], exact[k]) for k in ("out", "dx", "dW_ih"))   # the selector is wired


# ---- 4. without a gradient for x (no gru_dx_b3 launch), and for hxs
@pytest.mark.parametrize("products", PRODUCTS)
@pytest.mark.parametrize("x_grad,h_grad", [(False, True), (True, False)])
def test_without_an_input_gradient(L, products, x_grad, h_grad):
    N, T = 17, 3
    inp = U.edge_inputs(N, T)
    f64, ref = refs((N, T), inp, N, T)
    layer = device_layer(L, inp, products)
    part, full = run(layer, inp, x_grad=x_grad, h_grad=h_grad), run(layer, inp)
    assert ("dx" in part) == x_grad and ("dhxs" in part) == h_grad and len(part) == len(U.KEYS) - 1
    held(f"x_grad={x_grad} h_grad={h_grad}", products, part, ref, f64, keys=tuple(part))
    for k in part:
        assert np.array_equal(part[k], full[k]), k   # what is computed does not depend on what else is


# ---- 5. the default is untouched
def test_default_is_the_fp32_form(L, pkg):
    TC = importlib.import_module("aircombat-selfplay_amd.train_common")
    N, T, H = 37, 5, U.H
    M = N * T
    inp = U.edge_inputs(N, T)
    c = lambda k, g=False: torch.tensor(inp[k], device="cuda", requires_grad=g)
    p = [c(k, True) for k in U.GRU_NAMES + U.NORM_NAMES]
    res = {}
    for tag, kw in (("old", {}), ("named", {"dense_products": "fp32"}), ("split", {"dense_products": "bf16x3"})):
        x, hxs = c("x", True), c("hxs", True)
        for t in p:
            t.grad = None
        out, h_T = L.gru_layer(x, hxs.reshape(N, H), c("masks").reshape(M), *p, **kw)
        ((out * c("g_out")).sum() + (h_T * c("g_h").reshape(N, H)).sum()).backward()
        res[tag] = [out.detach(), h_T.detach(), x.grad, hxs.grad] + [t.grad.clone() for t in p]
    assert all(torch.equal(a, b) for a, b in zip(res["old"], res["named"]))
    assert not torch.equal(res["old"][0], res["split"][0]) and not torch.equal(res["old"][2], res["split"][2])   # and the option is live
    # the `_p` entry, and the `_pd` entry with AC_PRODUCTS_FP32
    x, hxs, masks, g_out, g_h = c("x"), c("hxs").reshape(N, H).contiguous(), c("masks").reshape(M), c("g_out"), c("g_h").reshape(N, H).contiguous()
    w_ih, w_hh, b_ih, b_hh, gamma, beta = (t.detach() for t in p)
    run_ = TC.Launch(x)
    new = lambda *s: torch.full(s, float("nan"), device="cuda")
    for sfx, tail in (("_p", (0,)), ("_pd", (0, 0))):
        out, h2, y2, saved2, stats = new(M, H), new(N, H), new(M, H), new(M, 4 * H), new(M, 2)
        run_("ac_gru_layer_forward" + sfx, N, T, x, hxs, masks, w_ih, w_hh, b_ih, b_hh, gamma, beta, 1e-5, new(M * 3 * H), out, h2, y2, saved2, stats, *tail)
        ws = run_.workspace("ac_gru_layer_workspace_floats", N, T)
        grads = [new(M, H), new(N, H), new(3 * H, H), new(3 * H, H), new(3 * H), new(3 * H), new(H), new(H)]
        run_("ac_gru_layer_backward" + sfx, N, T, g_out, g_h, x, hxs, masks, w_ih, w_hh, gamma, y2, saved2, stats, ws, *grads, *tail)
        torch.cuda.synchronize()
        got = [out, h2] + grads
        assert all(torch.equal(a.reshape(b.shape), b) for a, b in zip(res["old"], got)), sfx


# ---- 6. determinism, 7. stream discipline
@pytest.mark.parametrize("products", PRODUCTS)
def test_determinism(L, products):
    N, T, inp = _long()
    a = run(device_layer(L, inp, products), inp)
    b = run(device_layer(L, inp, products), inp)
    for k in U.KEYS:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("products", PRODUCTS)
def test_side_stream(L, products):
    inp = {**GU.inputs("mix"), **U.affine(95)}
    layer = device_layer(L, inp, products)
    base = run(layer, inp)
    c = lambda k, g=False: torch.tensor(inp[k], dtype=torch.float32, device="cuda", requires_grad=g)
    x0, hxs, masks, g_out = c("x"), c("hxs", True), c("masks"), c("g_out")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        x = (x0 * 2.0).requires_grad_()   # a dependent torch op before the layer ..
        out, _ = layer(x * 0.5, hxs, masks)
        after = out * 2.0                 # .. and after it
        (after * g_out).sum().backward()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(after.detach().double().cpu().numpy(), base["out"] * 2.0)
    assert torch.isfinite(x.grad).all() and torch.isfinite(layer.gru.weight_ih_l0.grad).all()


# ---- 8. all-zero and all-one masks
@pytest.mark.parametrize("products", PRODUCTS)
@pytest.mark.parametrize("value", [0.0, 1.0])
def test_uniform_masks(L, products, value):
    N, T = 33, 3
    inp = U.edge_inputs(N, T)
    inp["masks"] = np.full_like(inp["masks"], value)
    f64, ref = refs(("masks", value), inp, N, T)
    split = run(device_layer(L, inp, products), inp)
    held(f"masks {value:g}", products, split, ref, f64)
    if value == 0.0:   # h_in is zero at every step: nothing reaches W_hh or hxs
        assert not split["dW_hh"].any() and not split["dhxs"].any() and split["dW_ih"].any()


# ---- 9. a whole PPO update
def _flat(ts):
    return torch.cat([t.detach().double().reshape(-1) for t in ts]).cpu().numpy()


def test_whole_ppo_update(L, pkg):
    buf, nchunks, chunk = U.filled_buffer(pkg)
    sample = U.first_sample(buf, nchunks, chunk)
    base = U.Policy(seed=11)
    runs = {}
    for kind in ("torch", "f64", "off", "on"):
        pol, s = copy.deepcopy(base), sample
        if kind == "f64":
            pol.actor.double(); pol.critic.double()
            s = tuple(t.double() for t in sample)
        if kind in ("off", "on"):
            form = "bf16x3" if kind == "on" else "fp32"
            assert L.use_device_gru_layer(pol, products=form, dense_products=form) == 2
            assert pol.actor.rnn.dense_products == pol.critic.rnn.dense_products == form
            assert pkg.use_device_mlp(pol) == 4 and pkg.use_device_act(pol) == 1
            ret = pkg.DevicePPOTrainer(U.trainer_args(), torch.device("cuda", 0)).ppo_update(pol, sample)
            assert len(ret) == 6 and all(torch.isfinite(x).all() for x in ret)
        else:
            U.ppo_update(pol, s)
        params = list(pol.actor.parameters()) + list(pol.critic.parameters())
        runs[kind] = (_flat([p.grad for p in params]), _flat(params))
    for i, what in enumerate(("gradients", "parameters")):
        e_on, e_off, e_ref = (rel(runs[k][i], runs["f64"][i]) for k in ("on", "off", "torch"))
        assert np.isfinite(runs["on"][i]).all()
        print(f"ppo update {what}: both selectors on {e_on:.2e}, both off {e_off:.2e}, torch fp32 {e_ref:.2e}")
        assert e_on <= bound(e_ref), (what, e_on, e_ref)   # the bound the update with both off is held to
