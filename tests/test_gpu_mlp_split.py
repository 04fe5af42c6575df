"""The training MLP blocks' opt-in split-bf16 products (products="bf16x3": csrc/mlp_train_split.hpp) on the MI355X, every test under both
``products``: against the reference's float64 MLPLayer (tests/golden/mlp_train.npz), against float64 torch at the tile edges in M and
in K and over 1032 tiles with several per workgroup, with and without a gradient for x, the untouched default, determinism, stream
discipline, the C entries' refusal of an unknown code and a whole PPO update.

The bound everywhere is gru_split_util's: with rel(a, ref) = max|a - ref| / max|ref| against float64, rel(device) <=
max(4 * rel(torch fp32), 2^-20), where torch fp32 is the same modules in eager torch on the same GPU and inputs.

The ReLU is discontinuous in the backward: a pre-activation within rounding of 0 can get a different mask in fp32 and in float64, and
its row's gradients then differ by a whole term. The golden cases have no such pre-activation (test_mlp_split_host.py). Where the
inputs are random (``near_zero_rows``), z of both blocks is computed in float64 first and g_out is zeroed on every row that has a
|z64| below 2^-14: such a row's dz is 0 whatever the mask, in all three computations alike. The forward results are compared on all
rows."""
import copy
import importlib

import numpy as np
import pytest

import act_train_util as AU
import mlp_split_util as S
import mlp_train_util as U
from mlp_split_util import PRODUCTS, bound, rel

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
nn = torch.nn
NEAR = 2.0 ** -14


@pytest.fixture(scope="module")
def Mt(pkg):
    return importlib.import_module("aircombat-selfplay_amd.mlp_train")


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def layer_from(inp, dtype=torch.float32):
    m = U.MLP(inp["fc.0.weight"].shape[1]).cuda().to(dtype)
    m.load_state_dict({k: torch.as_tensor(inp[k]).to(dtype) for k in U.PNAMES})
    return m


def device_layer(Mt, inp, products):
    holder = nn.Module()
    holder.mlp = layer_from(inp)
    fc = holder.mlp.fc
    assert Mt.use_device_mlp(holder, products=products) == 1
    assert type(holder.mlp) is Mt.DeviceMLPLayer and holder.mlp.fc is fc and holder.mlp.products == products
    return holder.mlp


def run(layer_fn, mlp, inp, x_grad=True, dtype=torch.float32):
    params = dict(mlp.named_parameters())
    for p in params.values():
        p.grad = None
    x = torch.as_tensor(inp["x"]).to("cuda", dtype).requires_grad_(x_grad)
    return U.run_with_grads(layer_fn, params, x, torch.as_tensor(inp["g_out"]).to("cuda", dtype))


def device_layer_fn(Mt, dev):
    """(y0, y1) of a swapped layer through its blocks, as DeviceMLPLayer.forward chains them (test_layer_is_the_chain_of_its_blocks)."""
    fc = dev.fc
    def fn(x):
        y0 = Mt.mlp_block(x, fc[0], fc[2], products=dev.products)
        return y0, Mt.mlp_block(y0, fc[3], fc[5], products=dev.products)
    return fn


def run_device(Mt, inp, products, x_grad=True):
    dev = device_layer(Mt, inp, products)
    return run(device_layer_fn(Mt, dev), dev, inp, x_grad)


def run_torch(inp, x_grad=True, dtype=torch.float32):
    ref = layer_from(inp, dtype)
    return run(U.module_layer_fn(ref), ref, inp, x_grad, dtype)


def near_zero_rows(inp):
    """bool [M]: the rows that have a float64 pre-activation of either block below 2^-14 in magnitude."""
    m = layer_from(inp, torch.float64)
    with torch.no_grad():
        x = torch.as_tensor(inp["x"]).to("cuda", torch.float64)
        z0 = m.fc[0](x)
        z1 = m.fc[3](m.fc[2](torch.relu(z0)))
        return ((z0.abs() < NEAR).any(1) | (z1.abs() < NEAR).any(1)).cpu().numpy()


def treated(inp):
    """(inputs with g_out zeroed on near_zero_rows, the share of such rows)"""
    rows = near_zero_rows(inp)
    out = dict(inp, g_out=inp["g_out"].copy())
    out["g_out"][rows] = 0.0
    return out, float(rows.mean())


_refs = {}


def refs(tag, inp, x_grad=True):
    """(float64, torch fp32) of a case, computed once and shared."""
    if tag not in _refs:
        _refs[tag] = (run_torch(inp, x_grad, torch.float64), run_torch(inp, x_grad))
    return _refs[tag]


def held(what, products, dev, ref, f64, keys=None, pick=lambda k, a: a):
    bad = []
    for k in (keys if keys is not None else tuple(dev)):
        assert np.isfinite(dev[k]).all(), (what, k)
        e_dev, e_ref = rel(pick(k, dev[k]), f64[k]), rel(pick(k, ref[k]), f64[k])
        print(f"{what} products={products} {k}: device {e_dev:.2e}, torch fp32 {e_ref:.2e}, bound {bound(e_ref):.2e}")
        if not e_dev <= bound(e_ref):
            bad.append((k, e_dev, e_ref))
    assert not bad, (what, products, bad)


def runs_split(lib, K):
    return bool(lib.ac_mlp_block_constant(3) & S.split_kp(K))


# ---- 1. the golden cases
@pytest.mark.parametrize("products", PRODUCTS)
@pytest.mark.parametrize("name", list(U.CASES))
def test_golden_agreement(Mt, name, products):
    g, inp, x_grad = U.golden(), U.inputs(name), U.CASES[name][2]
    dev, ref = run_device(Mt, inp, products, x_grad), run_torch(inp, x_grad)
    assert set(dev) == set(U.keys(name))
    held(f"golden {name}", products, dev, ref, {k: g[f"{name}/{k}"] for k in U.keys(name)}, keys=U.keys(name), pick=U.stored)
    if name == "dead":
        dead = list(U.DEAD_ROWS)
        beta = np.broadcast_to(inp["fc.2.bias"].astype(np.float64), (len(dead), 128))
        assert np.array_equal(dev["y0"][dead], beta)   # relu(z) all zero, variance 0: y = beta bit for bit


@pytest.mark.parametrize("products", PRODUCTS)
def test_layer_is_the_chain_of_its_blocks(Mt, products):
    inp = U.inputs("obs15")
    dev = device_layer(Mt, inp, products)
    x = torch.as_tensor(inp["x"]).cuda()
    y = dev(x)
    assert y.grad_fn is not None and torch.equal(y, device_layer_fn(Mt, dev)(x)[1])
    with torch.no_grad():   # the inference form of the forward (no statistics kept) gives the same y
        assert torch.equal(dev(x), y)


# ---- 2. the tile edges in M
@pytest.mark.parametrize("products", PRODUCTS)
@pytest.mark.parametrize("M", [1, 31, 32, 33, 64, 65])
def test_tile_edges_in_m(Mt, M, products):
    inp, share = treated(S.edge_inputs(M, 128))
    assert share <= (0.0 if M == 1 else 0.1), share   # the comparison of the gradients is not empty
    f64, ref = refs(("M", M), inp)
    held(f"edge M = {M}", products, run_device(Mt, inp, products), ref, f64, keys=U.KEYS)


# ---- 3. the edges in K: KP = 32 (K 1, 12, 15 unaligned, 32), 64 (33, 64), 128 (65, 128), 256 (129, 168, 256)
def _single_block(Mt, inp, products):
    lin, norm = nn.Linear(inp["x"].shape[1], 128).cuda(), nn.LayerNorm(128).cuda()
    lin.load_state_dict({"weight": torch.as_tensor(inp["fc.0.weight"]), "bias": torch.as_tensor(inp["fc.0.bias"])})
    norm.load_state_dict({"weight": torch.as_tensor(inp["fc.2.weight"]), "bias": torch.as_tensor(inp["fc.2.bias"])})
    x = torch.as_tensor(inp["x"]).cuda().requires_grad_()
    y = Mt.mlp_block(x, lin, norm, products=products)
    (y * torch.as_tensor(inp["g_out"]).cuda()).sum().backward()
    return [y.detach(), x.grad] + [p.grad for p in list(lin.parameters()) + list(norm.parameters())]


@pytest.mark.parametrize("products", PRODUCTS)
@pytest.mark.parametrize("K", [1, 12, 15, 32, 33, 64, 65, 128, 129, 168, 256])
def test_edges_in_k(Mt, lib, K, products):
    M = 33
    inp, share = treated(S.edge_inputs(M, K))
    assert share <= 0.1, share
    f64, ref = refs(("K", K), inp)
    full, part = run_device(Mt, inp, products), run_device(Mt, inp, products, x_grad=False)
    held(f"edge K = {K}", products, full, ref, f64, keys=U.KEYS)
    assert set(part) == set(U.KEYS) - {"dx0"}   # without a gradient for x: no dx ..
    for k in part:
        assert np.array_equal(part[k], full[k]), k   # .. and what is computed does not depend on what else is
    if products == "bf16x3" and not runs_split(lib, K):   # the fp32 kernels run there: one block alone is theirs bit for bit
        assert all(torch.equal(a, b) for a, b in zip(_single_block(Mt, inp, "bf16x3"), _single_block(Mt, inp, "fp32")))


# ---- 4. several tiles per workgroup: 1032 tiles, a partial last one
BIG_M = 33000
_big = {}


def _big_case(K):
    if K not in _big:
        inp, share = treated(S.edge_inputs(BIG_M, K))
        x_grad = K == 128
        _big[K] = (inp, share, x_grad, run_torch(inp, x_grad, torch.float64), run_torch(inp, x_grad))
    return _big[K]


@pytest.mark.parametrize("products", PRODUCTS)
@pytest.mark.parametrize("K", [128, 15])
def test_several_tiles_per_workgroup(Mt, lib, K, products):
    tiles = -(-BIG_M // lib.ac_mlp_block_constant(0))
    assert tiles == 1032 and BIG_M % lib.ac_mlp_block_constant(0) != 0
    assert tiles > 2 * lib.ac_mlp_block_constant(1) and tiles > 4 * lib.ac_mlp_block_constant(2)
    inp, share, x_grad, f64, ref = _big_case(K)
    print(f"M = {BIG_M}, K = {K}: {100 * share:.2f} % of the rows have a |z64| below 2^-14")
    assert share <= 0.02
    dev = run_device(Mt, inp, products, x_grad)
    assert ("dx0" in dev) == x_grad
    held(f"1032 tiles K = {K}", products, dev, ref, f64)
    if products == "bf16x3" and runs_split(lib, K):
        exact = run_device(Mt, inp, "fp32", x_grad)
        assert any(not np.array_equal(dev[k], exact[k]) for k in ("y1", "dx0", "dW0") if k in dev)   # the selector is wired


# ---- 5. the default is the fp32 form, and the calls that existed before
def test_default_is_the_fp32_form(Mt, pkg):
    TC = importlib.import_module("aircombat-selfplay_amd.train_common")
    M, K = 77, 15
    inp = S.edge_inputs(M, K)
    c = lambda k, g=False: torch.tensor(inp[k], device="cuda", requires_grad=g)
    lin, norm = nn.Linear(K, 128).cuda(), nn.LayerNorm(128).cuda()
    lin.load_state_dict({"weight": c("fc.0.weight"), "bias": c("fc.0.bias")})
    norm.load_state_dict({"weight": c("fc.2.weight"), "bias": c("fc.2.bias")})
    p = list(lin.parameters()) + list(norm.parameters())
    res = {}
    for tag, kw in (("old", {}), ("named", {"products": "fp32"}), ("split", {"products": "bf16x3"})):
        x = c("x", True)
        for t in p:
            t.grad = None
        y = Mt.mlp_block(x, lin, norm, **kw)
        (y * c("g_out")).sum().backward()
        res[tag] = [y.detach(), x.grad] + [t.grad.clone() for t in p]
    assert all(torch.equal(a, b) for a, b in zip(res["old"], res["named"]))
    # the calls without `products`, and the `_p` calls with AC_PRODUCTS_FP32
    x, g_out = c("x"), c("g_out")
    w, b, gamma, beta = (t.detach() for t in p)
    run_ = TC.Launch(x)
    new = lambda *s: torch.full(s, float("nan"), device="cuda")
    for sfx, tail in (("", ()), ("_p", (0,))):
        y, stats = new(M, 128), new(M, 2)
        run_("ac_mlp_block_forward" + sfx, M, K, 1e-5, x, w, b, gamma, beta, y, stats, *tail)
        ws = run_.workspace("ac_mlp_block_workspace_floats", M, K)
        grads = [new(M, K), new(128, K), new(128), new(128), new(128)]
        run_("ac_mlp_block_backward" + sfx, M, K, g_out, x, w, b, gamma, stats, ws, *grads, *tail)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b_) for a, b_ in zip(res["old"], [y] + grads)), sfx


# ---- 6. determinism, on a side stream too
@pytest.mark.parametrize("products", PRODUCTS)
def test_determinism(Mt, products):
    for inp, x_grad in ((U.inputs("wide"), True), (_big_case(128)[0], True), (_big_case(15)[0], False)):
        a, b = run_device(Mt, inp, products, x_grad), run_device(Mt, inp, products, x_grad)
        assert set(a) == set(U.KEYS) - (set() if x_grad else {"dx0"})
        for k in a:
            assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("products", PRODUCTS)
def test_side_stream(Mt, products):
    inp = U.inputs("wide")
    base = run_device(Mt, inp, products)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = run_device(Mt, inp, products)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for k in U.KEYS:
        assert np.array_equal(base[k], side[k]), k


# ---- 7. an unknown code at the C entries
def test_unknown_products_code(lib):
    M, K = 8, 12
    t = lambda *s: torch.full(s, 7.0, device="cuda")
    o = lambda *s: torch.full(s, -3.0, device="cuda")   # outputs
    x, w, b, gm, bt, dy = t(M, K), t(128, K), t(128), t(128), t(128), t(M, 128)
    y, stats, ws, dx, dw, db, dg, dbe = o(M, 128), o(M, 2), o(128 * K + 384), o(M, K), o(128, K), o(128), o(128), o(128)
    stream = torch.cuda.current_stream().cuda_stream
    P = lambda v: v.data_ptr()
    for code in (2, -1, 7):
        assert lib.ac_mlp_block_forward_p(0, stream, M, K, 1e-5, P(x), P(w), P(b), P(gm), P(bt), P(y), P(stats), code) == -1
        assert "ac_mlp_block_forward_p: unknown products " + str(code) in lib.last_error()
        assert lib.ac_mlp_block_backward_p(0, stream, M, K, P(dy), P(x), P(w), P(b), P(gm), P(stats), P(ws), P(dx), P(dw), P(db), P(dg), P(dbe), code) == -1
        assert "ac_mlp_block_backward_p: unknown products " + str(code) in lib.last_error()
    torch.cuda.synchronize()
    assert all(bool((v == -3.0).all()) for v in (y, stats, ws, dx, dw, db, dg, dbe))   # nothing was launched
    for code in (0, 1):   # and the same buffers are accepted with a known one
        assert lib.ac_mlp_block_forward_p(0, stream, M, K, 1e-5, P(x), P(w), P(b), P(gm), P(bt), P(y), P(stats), code) == 0
        assert lib.ac_mlp_block_backward_p(0, stream, M, K, P(dy), P(x), P(w), P(b), P(gm), P(stats), P(ws), P(dx), P(dw), P(db), P(dg), P(dbe), code) == 0
        torch.cuda.synchronize()
        # constant rows: relu(z) = 7 * 7 * 12 + 7 in every unit (exact in either form), variance 0, so y = beta = 7 exactly
        assert bool((y == 7.0).all()) and all(torch.isfinite(v).all() and not bool((v == -3.0).any()) for v in (stats, dx, dw, db, dg, dbe))


# ---- 8. a whole PPO update
def _flat(ts):
    return torch.cat([t.detach().double().reshape(-1) for t in ts]).cpu().numpy()


def _filled_buffer(pkg, shared, T=32, E=32, L=8, seed=5):
    import types
    OBS, NVEC = U.OBS, U.NVEC
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


def _losses(policy, sample, shared, clip=0.2):
    """(policy loss, value loss, entropy) of mlp_train_util.ppo_update, before its step"""
    if shared:
        obs, cent, actions, masks, active, old_logp, adv, returns, vpreds, rnn_a, rnn_c = sample
    else:
        obs, actions, masks, old_logp, adv, returns, vpreds, rnn_a, rnn_c = sample
        cent, active = obs, torch.ones_like(masks)
    with torch.no_grad():
        values, logp, ent = policy.evaluate_actions(cent, obs, rnn_a, rnn_c, actions, masks)
        ratio = torch.exp(logp - old_logp)
        surr = torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv)
        policy_loss = -(torch.sum(surr, dim=-1, keepdim=True) * active).sum() / active.sum()
        vclip = vpreds + (values - vpreds).clamp(-clip, clip)
        value_loss = ((0.5 * torch.max((values - returns).pow(2), (vclip - returns).pow(2))) * active).sum() / active.sum()
        return _flat([policy_loss, value_loss, ent.mean()])


@pytest.mark.parametrize("shared", [False, True], ids=["own-obs", "share-obs"])
def test_whole_ppo_update(Mt, pkg, shared):
    """Held to what test_gpu_mlp_train.py::test_whole_ppo_update demands of the fp32 form: rel <= max(4 * torch fp32's, 2^-20) against
    the float64 update, for the gradients, the parameters after the step and the losses."""
    L = importlib.import_module("aircombat-selfplay_amd.gru_layer_train")
    buf, nchunks, chunk = _filled_buffer(pkg, shared, seed=5 + shared)
    order = np.random.default_rng(0).permutation(nchunks)
    sample = next(buf.recurrent_generator(buf.advantages if shared else buf, 1, chunk, chunk_order=order, on_device=True))
    base = AU.Policy(seed=11, critic_obs=2 * U.OBS if shared else U.OBS)
    runs = {}
    for kind in ("torch", "f64", "fp32", "bf16x3"):
        pol, s = copy.deepcopy(base), sample
        if kind == "f64":
            pol.actor.double(); pol.critic.double()
            s = tuple(t.double() for t in sample)
        if kind in PRODUCTS:
            assert L.use_device_gru_layer(pol) == 2 and Mt.use_device_mlp(pol, products=kind) == 4 and pkg.use_device_act(pol) == 1
            layers = [m for m in list(pol.actor.modules()) + list(pol.critic.modules()) if isinstance(m, Mt.DeviceMLPLayer)]
            assert len(layers) == 4 and all(m.products == kind for m in layers)
        losses = _losses(pol, s, shared)
        U.ppo_update(pol, s, shared=shared)
        params = list(pol.actor.parameters()) + list(pol.critic.parameters())
        runs[kind] = (_flat([p.grad for p in params]), _flat(params), losses)
    for i, what in enumerate(("gradients", "parameters", "losses")):
        e_on, e_off, e_ref = (rel(runs[k][i], runs["f64"][i]) for k in ("bf16x3", "fp32", "torch"))
        assert np.isfinite(runs["bf16x3"][i]).all()
        print(f"ppo update ({'share_obs' if shared else 'own obs'}) {what}: bf16x3 {e_on:.2e}, fp32 kernels {e_off:.2e}, torch fp32 {e_ref:.2e}, "
              f"bound {bound(e_ref):.2e}")
        # measured, bf16x3 / fp32 kernels / torch fp32: gradients 3.3e-7 / 3.4e-7 / 2.6e-7, parameters 1.2e-7 / 1.9e-7 /
        # 1.8e-7, losses 2.1e-8 all; share-obs 2.9e-7 / 3.3e-7 / 2.6e-7, 1.6e-7 / 2.3e-7 / 1.8e-7, 4.8e-8 all: no extra room is needed
        assert e_on <= bound(e_ref), (what, e_on, e_ref)
