"""The training GRU's opt-in split-bf16 product (products="bf16x3": csrc/gru_train_split.hpp) on the MI355X, through DeviceGRULayer
("seq": the recurrence kernels, the rest torch) and DeviceFusedGRULayer ("fused"): against the reference's float64 GRULayer
(tests/golden/gru_train.npz), against the tests' float64 restatement at the tile edges and over 60 steps on several workgroups, its
masks, its range, the untouched default, determinism, stream discipline and a whole PPO update.

The bound everywhere is test_gpu_gru_train.py's: with rel(a, ref) = max|a - ref| / max|ref| against float64, rel(bf16x3) <=
max(4 * rel(torch fp32), 2^-20), where torch fp32 is the reference-form layer (segment_layer with nn.GRU and nn.LayerNorm) on the same GPU
and inputs. The exact-fp32 device form's error is printed beside it, for the record."""
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
KINDS = ("seq", "fused")


@pytest.fixture(scope="module")
def G(pkg):
    return importlib.import_module("aircombat-selfplay_amd.gru_train")


@pytest.fixture(scope="module")
def L(pkg):
    return importlib.import_module("aircombat-selfplay_amd.gru_layer_train")


@pytest.fixture(scope="module")
def mods(G, L):
    return {"seq": G, "fused": L}


def device_layer(mods, kind, inp, products="bf16x3"):
    """The case's layer swapped for the device layer of ``kind`` with ``products``."""
    holder = nn.Module()
    holder.rnn = U.layer_from(inp)
    if kind == "seq":
        assert mods["seq"].use_device_gru(holder, products=products) == 1 and type(holder.rnn) is mods["seq"].DeviceGRULayer
    else:
        assert mods["fused"].use_device_gru_layer(holder, products=products) == 1 and type(holder.rnn) is mods["fused"].DeviceFusedGRULayer
    assert holder.rnn.products == products
    return holder.rnn


def keys_of(kind):
    return GU.KEYS if kind == "seq" else U.KEYS


def run(layer, inp, over=None):
    src = dict(inp, **(over or {}))
    c = lambda k, g=False: torch.tensor(src[k], dtype=torch.float32, device="cuda", requires_grad=g)
    params = U.layer_params(layer)
    for p in params.values():
        p.grad = None
    return U.run_with_grads(layer, params, c("x", True), c("hxs", True), c("masks"), c("g_out"), c("g_h"))


def run_f64(inp, N, T):
    names = U.GRU_NAMES + tuple(k for k in U.NORM_NAMES if k in inp)
    p = {k: torch.tensor(inp[k], dtype=torch.float64, device="cuda", requires_grad=True) for k in names}
    c = lambda k, g=False: torch.tensor(inp[k], dtype=torch.float64, device="cuda", requires_grad=g)
    return U.run_with_grads(lambda x, h, m: U.step_layer(p, x, h, m, N, T), p, c("x", True), c("hxs", True), c("masks"), c("g_out"), c("g_h"))


def held(what, kind, split, exact, ref, f64, keys=None, pick=lambda k, a: a):
    for k in keys or keys_of(kind):
        assert np.isfinite(split[k]).all(), (what, k)
        e_dev, e_fp32, e_ref = (rel(pick(k, r[k]), f64[k]) for r in (split, exact, ref))
        print(f"{what} {kind} {k}: bf16x3 {e_dev:.2e}, device fp32 {e_fp32:.2e}, torch fp32 {e_ref:.2e}")
        assert e_dev <= bound(e_ref), (what, kind, k, e_dev, e_ref)


def legs(mods, kind, inp):
    return run(device_layer(mods, kind, inp), inp), run(device_layer(mods, kind, inp, "fp32"), inp), run(U.layer_from(inp), inp)


# ---- 1. the golden cases
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(GU.CASES))
def test_golden_agreement(mods, name, kind):
    g, inp = GU.golden(), GU.inputs(name)   # no norm.weight / norm.bias: the LayerNorm keeps its unit scale and zero shift
    gold = {k: g[f"{name}/{k}"] for k in GU.KEYS}
    held(f"golden {name}", kind, *legs(mods, kind, inp), gold, keys=GU.KEYS, pick=GU.stored)


# ---- 2. the tile edges, 3. sixty steps on several workgroups
_f64 = {}


def f64_of(tag, inp, N, T):
    if tag not in _f64:
        _f64[tag] = run_f64(inp, N, T)
    return _f64[tag]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("N", [15, 16, 17, 33])
def test_tile_edges(mods, N, T, kind):
    inp = U.edge_inputs(N, T)
    m = inp["masks"].reshape(T, N)
    assert (m[0] == 0).any() and (T < 3 or (m == 0).all(axis=1).any())
    held(f"edge {N} x {T}", kind, *legs(mods, kind, inp), f64_of((N, T), inp, N, T))


@pytest.mark.parametrize("kind", KINDS)
def test_sixty_steps_on_several_workgroups(mods, kind):
    N, T = 272, 60
    inp = U.random_inputs(N, T, done=0.02)
    assert (inp["masks"] == 0).any()
    held(f"recurrence {N} x {T}", kind, *legs(mods, kind, inp), f64_of("long", inp, N, T))


# ---- 4. masks
@pytest.mark.parametrize("kind", KINDS)
def test_masked_first_step_forgets_hxs(mods, kind):
    N, T, _ = GU.CASES["mix"]
    inp = {**GU.inputs("mix"), **U.affine(91)}
    masks = inp["masks"].copy().reshape(T, N)
    masks[0] = 0.0
    layer = device_layer(mods, kind, inp)
    a = run(layer, inp, {"masks": masks.reshape(T * N, 1)})
    b = run(layer, inp, {"masks": masks.reshape(T * N, 1), "hxs": -3.0 * inp["hxs"][::-1].copy() + 0.5})
    for k in keys_of(kind):
        assert np.array_equal(a[k], b[k]), k
    assert not a["dhxs"].any() and a["dx"].any()


@pytest.mark.parametrize("kind", KINDS)
def test_masked_step_cuts_the_chunk(mods, kind):
    N, T, _ = GU.CASES["mix"]
    inp = {**GU.inputs("mix"), **U.affine(92)}
    cut = 4
    assert not inp["masks"].reshape(T, N)[cut].any()   # every row's episode ended there
    x2 = inp["x"].copy()
    x2[:cut * N] = 0.25 - x2[:cut * N][::-1]
    layer = device_layer(mods, kind, inp)
    a = run(layer, inp)
    b = run(layer, inp, {"x": x2, "hxs": 2.0 * inp["hxs"]})
    assert not np.array_equal(a["out"][:cut * N], b["out"][:cut * N])
    for k in ("out", "dx"):
        assert np.array_equal(a[k][cut * N:], b[k][cut * N:]), k
    assert np.array_equal(a["h_T"], b["h_T"])


# ---- 5. range: gradients far below and above fp16's range
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("log2", [-40, 20])
def test_gradient_range(mods, log2, kind):
    N, T, _ = GU.CASES["mix"]
    s = np.float32(2.0 ** log2)
    inp = GU.inputs("mix")
    inp.update(g_out=inp["g_out"] * s, g_h=inp["g_h"] * s)
    grads = tuple(k for k in GU.KEYS if k.startswith("d"))
    f64 = f64_of(("range", log2), inp, N, T)
    assert all(1e-3 * s < np.abs(f64[k]).max() < 1e5 * s for k in grads)
    held(f"range 2^{log2}", kind, *legs(mods, kind, inp), f64, keys=grads)


# ---- 6. the default is untouched
@pytest.mark.parametrize("kind", KINDS)
def test_default_is_the_fp32_form(mods, kind):
    inp = {**GU.inputs("mix"), **U.affine(93)}
    holder = nn.Module()
    holder.rnn = U.layer_from(inp)
    assert (mods["seq"].use_device_gru(holder) if kind == "seq" else mods["fused"].use_device_gru_layer(holder)) == 1   # as before the option
    assert holder.rnn.products == "fp32"
    old = run(holder.rnn, inp)
    new = run(device_layer(mods, kind, inp, "fp32"), inp)
    split = run(device_layer(mods, kind, inp, "bf16x3"), inp)
    for k in keys_of(kind):
        assert np.array_equal(old[k], new[k]), k
    assert not np.array_equal(old["out"], split["out"])   # and the option is live


def test_capi_fp32_is_the_old_entries(pkg):
    TC = importlib.import_module("aircombat-selfplay_amd.train_common")
    N, T, H = 37, 5, U.H
    M = N * T
    inp = U.edge_inputs(N, T)
    c = lambda k: torch.tensor(inp[k], device="cuda").contiguous()
    x, hxs, masks, g_out, g_h = c("x"), c("hxs").reshape(N, H), c("masks").reshape(M), c("g_out"), c("g_h").reshape(N, H)
    w_ih, w_hh, b_ih, b_hh, gamma, beta = (c(k) for k in U.GRU_NAMES + U.NORM_NAMES)
    run = TC.Launch(x)
    new = lambda *s: torch.full(s, float("nan"), device="cuda")
    gi = torch.addmm(b_ih, x, w_ih.t())
    res = {}
    for tag, sfx, tail in (("old", "", ()), ("fp32", "_p", (0,)), ("bf16x3", "_p", (1,))):
        y, h_T, saved, dgi, dgh, dhxs = new(M, H), new(N, H), new(M, 4 * H), new(M, 3 * H), new(M, 3 * H), new(N, H)
        run("ac_gru_seq_forward" + sfx, N, T, gi, hxs, masks, w_hh, b_hh, y, h_T, saved, *tail)
        run("ac_gru_seq_backward" + sfx, N, T, g_out, g_h, saved, y, hxs, masks, w_hh, dgi, dgh, dhxs, *tail)
        out, h2, y2, saved2, stats = new(M, H), new(N, H), new(M, H), new(M, 4 * H), new(M, 2)
        run("ac_gru_layer_forward" + sfx, N, T, x, hxs, masks, w_ih, w_hh, b_ih, b_hh, gamma, beta, 1e-5, new(M * 3 * H), out, h2, y2, saved2, stats,
            *tail)
        ws = run.workspace("ac_gru_layer_workspace_floats", N, T)
        grads = [new(M, H), new(N, H), new(3 * H, H), new(3 * H, H), new(3 * H), new(3 * H), new(H), new(H)]
        run("ac_gru_layer_backward" + sfx, N, T, g_out, g_h, x, hxs, masks, w_ih, w_hh, gamma, y2, saved2, stats, ws, *grads, *tail)
        torch.cuda.synchronize()
        res[tag] = [y, h_T, saved, dgi, dgh, dhxs, out, h2, y2, saved2, stats] + grads
        assert all(torch.isfinite(t).all() for t in res[tag])
    assert all(torch.equal(a, b) for a, b in zip(res["old"], res["fp32"]))
    assert not torch.equal(res["old"][0], res["bf16x3"][0]) and not torch.equal(res["old"][6], res["bf16x3"][6])


# ---- 7. determinism, 8. stream discipline
@pytest.mark.parametrize("kind", KINDS)
def test_determinism(mods, kind):
    inp = {**GU.inputs("mix"), **U.affine(94)}
    a = run(device_layer(mods, kind, inp), inp)
    b = run(device_layer(mods, kind, inp), inp)
    for k in keys_of(kind):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("kind", KINDS)
def test_side_stream(mods, kind):
    inp = {**GU.inputs("mix"), **U.affine(95)}
    layer = device_layer(mods, kind, inp)
    base = run(layer, inp)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = run(layer, inp)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for k in keys_of(kind):
        assert np.array_equal(base[k], side[k]), k


@pytest.mark.parametrize("kind", KINDS)
def test_no_host_synchronisation(mods, kind):
    inp = U.random_inputs(256, 60, seed=4)
    dev, ref = device_layer(mods, kind, inp), U.layer_from(inp)
    c = lambda k, g=False: torch.tensor(inp[k], device="cuda", requires_grad=g)
    x, h, m, go = c("x", True), c("hxs", True), c("masks"), c("g_out")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, hT = dev(x, h, m)
        (out * go).sum().backward()
        with pytest.raises(RuntimeError):   # the reference's algorithm synchronises (nonzero().cpu()): the check is live
            ref(x, h, m)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(x.grad).all() and torch.isfinite(h.grad).all() and torch.isfinite(dev.gru.weight_hh_l0.grad).all()


# ---- 9. a whole PPO update
def _flat(ts):
    return torch.cat([t.detach().double().reshape(-1) for t in ts]).cpu().numpy()


def test_whole_ppo_update(G, L, pkg):
    buf, nchunks, chunk = U.filled_buffer(pkg)
    sample = U.first_sample(buf, nchunks, chunk)
    base = U.Policy(seed=11)
    runs = {}
    for kind in ("torch", "f64", "seq", "layer", "all"):
        pol, s = copy.deepcopy(base), sample
        adam_params = [p for grp in pol.optimizer.param_groups for p in grp["params"]]
        if kind == "f64":
            pol.actor.double(); pol.critic.double()
            s = tuple(t.double() for t in sample)
        if kind in ("seq", "all"):
            assert G.use_device_gru(pol, products="bf16x3") == 2
        if kind in ("layer", "all"):
            assert L.use_device_gru_layer(pol, **({"products": "bf16x3"} if kind == "layer" else {})) == 2
            assert type(pol.actor.rnn) is L.DeviceFusedGRULayer and type(pol.critic.rnn) is L.DeviceFusedGRULayer
        if kind in ("seq", "layer", "all"):
            assert pol.actor.rnn.products == pol.critic.rnn.products == "bf16x3"
        if kind == "all":
            assert pkg.use_device_mlp(pol) == 4 and pkg.use_device_act(pol) == 1
            ret = pkg.DevicePPOTrainer(U.trainer_args(), torch.device("cuda", 0)).ppo_update(pol, sample)
            assert len(ret) == 6 and all(torch.isfinite(x).all() for x in ret)
        else:
            U.ppo_update(pol, s)
        params = list(pol.actor.parameters()) + list(pol.critic.parameters())
        assert [id(p) for p in adam_params] == [id(p) for p in params]
        assert all(p in pol.optimizer.state and "exp_avg" in pol.optimizer.state[p] for p in params)
        runs[kind] = (_flat([p.grad for p in params]), _flat(params))
    for kind in ("seq", "layer", "all"):
        for i, what in enumerate(("gradients", "parameters")):
            e_dev, e_ref = rel(runs[kind][i], runs["f64"][i]), rel(runs["torch"][i], runs["f64"][i])
            assert np.isfinite(runs[kind][i]).all()
            print(f"ppo update ({kind}, bf16x3) {what}: device {e_dev:.2e}, torch fp32 {e_ref:.2e}")
            assert e_dev <= bound(e_ref), (kind, what, e_dev, e_ref)
