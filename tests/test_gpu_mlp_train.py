"""The training MLP blocks (DeviceMLPLayer, csrc/mlp_train.hpp) on the MI355X: against the reference's float64 MLPLayer
(tests/golden/mlp_train.npz), against float64 torch at a user's size, inside a whole PPO update with the GRU swapped too, and their
determinism, stream and sync discipline.

The bound everywhere: with rel(a, ref) = max|a - ref| / max|ref| against float64, rel(device) <= max(4 * rel(torch fp32 eager on the
same GPU), 2^-20), the bound test_gpu_gru_train.py uses for the same kind of comparison."""
import copy
import importlib
import types

import numpy as np
import pytest

import mlp_train_util as U

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
nn = torch.nn
FLOOR = 2.0 ** -20


@pytest.fixture(scope="module")
def Mt(pkg):
    return importlib.import_module("aircombat-selfplay_amd.mlp_train")


@pytest.fixture(scope="module")
def Gt(pkg):
    return importlib.import_module("aircombat-selfplay_amd.gru_train")


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def layer_from(inp, dtype=torch.float32):
    m = U.MLP(inp["fc.0.weight"].shape[1]).cuda().to(dtype)
    m.load_state_dict({k: torch.as_tensor(inp[k]).to(dtype) for k in U.PNAMES})
    return m


def _swapped(Mt, layer):
    holder = nn.Module()
    holder.mlp = layer
    assert Mt.use_device_mlp(holder) == 1
    assert isinstance(holder.mlp, Mt.DeviceMLPLayer) and holder.mlp.fc is layer.fc
    return holder.mlp


def device_layer_fn(Mt, dev):
    """(y0, y1) of a swapped layer through its blocks, as DeviceMLPLayer.forward chains them (test_inference_path holds the two equal)."""
    fc = dev.fc
    def fn(x):
        y0 = Mt.mlp_block(x, fc[0], fc[2])
        return y0, Mt.mlp_block(y0, fc[3], fc[5])
    return fn


def run(layer_fn, mlp, inp, x_grad=True, dtype=torch.float32):
    params = dict(mlp.named_parameters())
    for p in params.values():
        p.grad = None
    x = torch.as_tensor(inp["x"]).to("cuda", dtype).requires_grad_(x_grad)
    return U.run_with_grads(layer_fn, params, x, torch.as_tensor(inp["g_out"]).to("cuda", dtype))


def run_device(Mt, inp, x_grad=True):
    dev = _swapped(Mt, layer_from(inp))
    return run(device_layer_fn(Mt, dev), dev, inp, x_grad)


def run_torch(inp, x_grad=True, dtype=torch.float32):
    ref = layer_from(inp, dtype)
    return run(U.module_layer_fn(ref), ref, inp, x_grad, dtype)


@pytest.mark.parametrize("name", list(U.CASES))
def test_golden_agreement(Mt, name):
    g, inp, x_grad = U.golden(), U.inputs(name), U.CASES[name][2]
    dev, ref = run_device(Mt, inp, x_grad), run_torch(inp, x_grad)
    assert set(dev) == set(U.keys(name))
    bad = []
    for k in U.keys(name):
        gold = g[f"{name}/{k}"]
        e_dev, e_ref = rel(U.stored(k, dev[k]), gold), rel(U.stored(k, ref[k]), gold)
        assert np.isfinite(dev[k]).all(), k
        print(f"golden {name} {k}: device {e_dev:.2e}, torch fp32 {e_ref:.2e}")
        if not e_dev <= max(4 * e_ref, FLOOR):
            bad.append((k, e_dev, e_ref))
    assert not bad, (name, bad)
    if name == "dead":
        dead = list(U.DEAD_ROWS)
        beta = np.broadcast_to(inp["fc.2.bias"].astype(np.float64), (len(dead), 128))
        assert np.array_equal(dev["y0"][dead], beta)   # relu(z) all zero, variance 0: y = beta bit for bit


def _big_inputs(M, K, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    inp = {"fc.0.weight": rn(128, K) / np.sqrt(K), "fc.0.bias": rn(128) * 0.1, "fc.2.weight": 1 + 0.3 * rn(128), "fc.2.bias": 0.3 * rn(128),
           "fc.3.weight": rn(128, 128) / np.sqrt(128), "fc.3.bias": rn(128) * 0.1, "fc.5.weight": 1 + 0.3 * rn(128), "fc.5.bias": 0.3 * rn(128),
           "x": rn(M, K), "g_out": rn(M, 128)}
    return {k: v.cpu().numpy() for k, v in inp.items()}


@pytest.mark.parametrize("K", [128, 15])
def test_parity_at_user_size(Mt, K):
    """One layer at M = 4096 x 60 rows against the same modules in float64 on the GPU: the parameter gradients are sums over 245 760
    rows here (256 workgroup partials of 960 rows each, then eight interleaved sums and a tree).

    Measured: y and, at K = 15, every gradient are 2e-7 to 7e-7 on the device. At K = 128 most gradients read 5e-4 to
    1e-1 for the device and for torch alike: a handful of the 31 million pre-activations lie within fp32 rounding of 0, where fp32 and
    float64 disagree about the ReLU mask, and one such unit moves its row of dx by a whole term. The worst ratio seen is 3.0 (dx1)."""
    M = 4096 * 60
    inp = _big_inputs(M, K, seed=7 + K)
    x_grad = K == 128
    dev = run_device(Mt, inp, x_grad)
    ref = run_torch(inp, x_grad)
    f64 = run_torch(inp, x_grad, torch.float64)
    bad = []
    for k in dev:
        assert np.isfinite(dev[k]).all(), k
        e_dev, e_ref = rel(dev[k], f64[k]), rel(ref[k], f64[k])
        print(f"parity 4096 x 60, K = {K}, {k}: device {e_dev:.2e}, torch fp32 {e_ref:.2e}")
        if not e_dev <= max(4 * e_ref, FLOOR):
            bad.append((k, e_dev, e_ref))
    assert not bad, (K, bad)


# ---- a whole PPO update on the restated policy (mlp_train_util), fed by an on-device minibatch
def _filled_buffer(pkg, shared=False, T=32, E=32, L=8, seed=5):
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


def _flat(ts):
    return torch.cat([t.detach().double().reshape(-1) for t in ts]).cpu().numpy()


@pytest.mark.parametrize("shared", [False, True], ids=["own-obs", "share-obs"])
def test_whole_ppo_update(Mt, Gt, pkg, shared):
    buf, nchunks, L = _filled_buffer(pkg, shared=shared, seed=5 + shared)
    order = np.random.default_rng(0).permutation(nchunks)
    gen = buf.recurrent_generator(buf.advantages, 1, L, chunk_order=order, on_device=True) if shared else \
        buf.recurrent_generator(buf, 1, L, chunk_order=order, on_device=True)
    sample = next(gen)
    assert all(isinstance(s, torch.Tensor) and s.is_cuda for s in sample)
    base = U.Policy(seed=11, critic_obs=2 * U.OBS if shared else U.OBS)
    assert base.critic.base.mlp.fc[0].in_features == (2 if shared else 1) * U.OBS
    runs = {}
    for kind in ("torch", "device", "f64"):
        pol = copy.deepcopy(base)
        if kind == "device":
            adam_params = [p for grp in pol.optimizer.param_groups for p in grp["params"]]
            assert Gt.use_device_gru(pol) == 2 and Mt.use_device_mlp(pol) == 4
            mods = list(pol.actor.modules()) + list(pol.critic.modules())
            assert sum(isinstance(m, Mt.DeviceMLPLayer) for m in mods) == 4 and sum(isinstance(m, Gt.DeviceGRULayer) for m in mods) == 2
            # the optimiser built before the swaps still holds the very Parameter objects the swapped modules use
            assert [id(p) for p in adam_params] == [id(p) for p in list(pol.actor.parameters()) + list(pol.critic.parameters())]
        s = sample
        if kind == "f64":
            pol.actor.double(); pol.critic.double()
            s = tuple(t.double() for t in sample)
        U.ppo_update(pol, s, shared=shared)
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


def test_determinism(Mt):
    for inp in (U.inputs("wide"), _big_inputs(4096 * 8, 128, seed=2)):
        a, b = run_device(Mt, inp), run_device(Mt, inp)
        assert set(a) == set(U.KEYS)
        for k in a:
            assert np.array_equal(a[k], b[k]), k


def test_no_host_synchronisation(Mt):
    inp = _big_inputs(512 * 60, 15, seed=4)
    dev = _swapped(Mt, layer_from(inp))
    x = torch.as_tensor(inp["x"]).cuda().requires_grad_(True)
    go = torch.as_tensor(inp["g_out"]).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = dev(x)
        (out * go).sum().backward()
        with pytest.raises(RuntimeError):   # a torch call that does synchronise raises under the same mode: the check is live
            out.sum().item()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(x.grad).all() and all(torch.isfinite(p.grad).all() for p in dev.parameters())


def test_side_stream(Mt):
    inp = U.inputs("wide")
    base = run_device(Mt, inp)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = run_device(Mt, inp)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for k in U.KEYS:
        assert np.array_equal(base[k], side[k]), k


def test_inference_path(Mt, monkeypatch):
    inp = U.inputs("obs15")
    dev = _swapped(Mt, layer_from(inp))
    x = torch.as_tensor(inp["x"]).cuda()
    saves = []
    fwd = Mt.DeviceMLPBlockFunction.forward
    monkeypatch.setattr(Mt.DeviceMLPBlockFunction, "forward", staticmethod(lambda ctx, *a: (saves.append(a[-1]), fwd(ctx, *a))[1]))
    y_grad = dev(x)
    assert saves == [True, True] and y_grad.grad_fn is not None
    y0, y1 = device_layer_fn(Mt, dev)(x)
    assert torch.equal(y1, y_grad)                      # the layer's forward is the chain of its blocks
    del saves[:]
    with torch.no_grad():
        y_ng = dev(x)
    assert saves == [False, False] and y_ng.grad_fn is None and not y_ng.requires_grad
    for p in dev.parameters():
        p.requires_grad_(False)
    y_frozen = dev(x)                                   # grad mode on, but nothing requires grad
    assert saves == [False] * 4 and y_frozen.grad_fn is None
    assert torch.equal(y_ng, y_grad) and torch.equal(y_frozen, y_grad)
    assert torch.equal(dev(x.view(7, 11, 15)), y_grad.view(7, 11, 128))   # leading dimensions are flattened and restored


def test_refusals_on_the_device(Mt, pkg):
    inp = U.inputs("one")
    x = torch.as_tensor(inp["x"]).cuda()
    dev = _swapped(Mt, layer_from(inp)).double()
    with pytest.raises(pkg.UnsupportedPolicy, match=r"fc\.0: dtype torch.float64"):
        dev(x.double())
    dev = _swapped(Mt, layer_from(inp)).cpu()
    with pytest.raises(pkg.UnsupportedPolicy, match=r"fc\.0: device cpu"):
        dev(x)
    dev = _swapped(Mt, layer_from(inp))
    with pytest.raises(pkg.UnsupportedPolicy, match="input torch.float64"):
        dev(x.double())
    # the C calls: refused with a message, nothing launched (the outputs keep their sentinel)
    lib = pkg.load_library()
    M, K = 8, 12
    t = lambda *s: torch.full(s, 7.0, device="cuda")
    o = lambda *s: torch.full(s, -3.0, device="cuda")   # outputs
    xx, w, b, gm, bt, dy = t(M, K), t(128, K), t(128), t(128), t(128), t(M, 128)
    y, stats, ws, dx, dw, db, dg, dbe = o(M, 128), o(M, 2), o(128 * K + 384), o(M, K), o(128, K), o(128), o(128), o(128)
    stream = torch.cuda.current_stream().cuda_stream
    P = lambda v: v.data_ptr()
    fwd = lambda M, K, xp=P(xx): lib.ac_mlp_block_forward(0, stream, M, K, 1e-5, xp, P(w), P(b), P(gm), P(bt), P(y), P(stats))
    bwd = lambda M, K, dyp=P(dy): lib.ac_mlp_block_backward(0, stream, M, K, dyp, P(xx), P(w), P(b), P(gm), P(stats), P(ws), P(dx), P(dw), P(db), P(dg), P(dbe))
    for call in (fwd, bwd):
        for args, what in (((M, 0), "K must be"), ((M, 257), "K must be"), ((0, K), "M must be"), ((M, K, None), "null argument")):
            assert call(*args) == -1 and what in lib.last_error(), (args, lib.last_error())
    torch.cuda.synchronize()
    assert all(bool((v == -3.0).all()) for v in (y, stats, ws, dx, dw, db, dg, dbe))
    assert fwd(M, K) == 0 and bwd(M, K) == 0        # and the same buffers are accepted when the arguments are in range
    torch.cuda.synchronize()
    # constant rows: relu(z) = 7 * 7 * 12 + 7 in every unit, variance 0, so y = beta = 7 exactly
    assert bool((y == 7.0).all()) and all(torch.isfinite(v).all() and not bool((v == -3.0).any()) for v in (stats, dx, dw, db, dg, dbe))
