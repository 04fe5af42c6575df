"""The whole GRU layer on the device (DeviceFusedGRULayer, csrc/gru_layer_train.hpp) on the MI355X: against the reference's float64
GRULayer (tests/golden/gru_train.npz), against the tests' float64 restatement with a non-trivial scale and shift at every tile edge, over
the kernels' persistent loops and partial sums, over the weight gradients' longest running sums, inside a whole PPO update, and its
gradient, stream and sync discipline.

The bound everywhere is test_gpu_gru_train.py's: with rel(a, ref) = max|a - ref| / max|ref| against float64, rel(device) <=
max(4 * rel(torch fp32), 2^-20), where torch fp32 is the reference-form layer (segment_layer with nn.GRU and nn.LayerNorm) on the same GPU
and inputs."""
import copy
import importlib

import numpy as np
import pytest

import gru_layer_util as U
import gru_train_util as GU

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
nn = torch.nn
FLOOR = 2.0 ** -20


@pytest.fixture(scope="module")
def L(pkg):
    return importlib.import_module("aircombat-selfplay_amd.gru_layer_train")


@pytest.fixture(scope="module")
def consts(pkg):
    lib = pkg.load_library()
    return [lib.ac_gru_layer_constant(i) for i in range(6)]


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def fused(L, layer):
    holder = nn.Module()
    holder.rnn = layer
    assert L.use_device_gru_layer(holder) == 1 and type(holder.rnn) is L.DeviceFusedGRULayer
    return holder.rnn


def run(layer, inp):
    c = lambda k, g=False: torch.tensor(inp[k], dtype=torch.float32, device="cuda", requires_grad=g)
    params = U.layer_params(layer)
    for p in params.values():
        p.grad = None
    return U.run_with_grads(layer, params, c("x", True), c("hxs", True), c("masks"), c("g_out"), c("g_h"))


def run_f64(inp, N, T):
    p = {k: torch.tensor(inp[k], dtype=torch.float64, device="cuda", requires_grad=True) for k in U.GRU_NAMES + U.NORM_NAMES}
    c = lambda k, g=False: torch.tensor(inp[k], dtype=torch.float64, device="cuda", requires_grad=g)
    return U.run_with_grads(lambda x, h, m: U.step_layer(p, x, h, m, N, T), p, c("x", True), c("hxs", True), c("masks"), c("g_out"), c("g_h"))


def held(what, dev, ref, f64, keys=U.KEYS):
    for k in keys:
        assert np.isfinite(dev[k]).all(), (what, k)
        e_dev, e_ref = rel(dev[k], f64[k]), rel(ref[k], f64[k])
        print(f"{what} {k}: device {e_dev:.2e}, torch fp32 {e_ref:.2e}")
        assert e_dev <= max(4 * e_ref, FLOOR), (what, k, e_dev, e_ref)


def three_legs(L, inp, N, T):
    return run(fused(L, U.layer_from(inp)), inp), run(U.layer_from(inp), inp), run_f64(inp, N, T)


@pytest.mark.parametrize("name", list(GU.CASES))
def test_golden_agreement(L, name):
    g, inp = GU.golden(), GU.inputs(name)   # no norm.weight / norm.bias: the LayerNorm keeps its unit scale and zero shift
    dev = run(fused(L, U.layer_from(inp)), inp)
    ref = run(U.layer_from(inp), inp)
    for k in GU.KEYS:
        gold = g[f"{name}/{k}"]
        e_dev, e_ref = rel(GU.stored(k, dev[k]), gold), rel(GU.stored(k, ref[k]), gold)
        assert np.isfinite(dev[k]).all(), k
        print(f"golden {name} {k}: device {e_dev:.2e}, torch fp32 {e_ref:.2e}")
        assert e_dev <= max(4 * e_ref, FLOOR), (name, k, e_dev, e_ref)


EDGES = ("1x1", "1x2", "R-1x1", "Rx1", "R+1x1", "R+1x3", "2R+1x2")


@pytest.mark.parametrize("edge", EDGES)
def test_affine_and_tile_edges(L, consts, edge):
    R = consts[0]
    n, T = edge.split("x")
    N, T = {"1": 1, "R-1": R - 1, "R": R, "R+1": R + 1, "2R+1": 2 * R + 1}[n], int(T)
    inp = U.edge_inputs(N, T)
    m = inp["masks"].reshape(T, N)
    assert (m[0] == 0).any() and (T == 1 or (m[1:] == 0).any()) and (T < 3 or (m == 0).all(axis=1).any())
    held(f"edge {N} x {T}", *three_legs(L, inp, N, T))


def test_persistent_loop_and_partials(L, consts):
    R, W = consts[0], max(consts[1:])
    N, T = R * W + 1, 2   # 2 R W + 2 rows: every workgroup of every kernel walks more than one tile, and the last tile has two rows
    assert all((N * T + R - 1) // R > 2 * w for w in consts[1:]) and (N * T) % R
    held(f"persistent {N} x {T}", *three_legs(L, U.random_inputs(N, T, done=0.3, seed=8), N, T))


def test_accumulation_length(L, consts):
    R, Wdw = consts[0], consts[4]
    T = 60
    N = -(-8 * R * Wdw // T)   # each workgroup of the weight-gradient kernel sums at least 8 tiles of rows
    assert (N * T) // R >= 8 * Wdw
    inp = U.random_inputs(N, T, done=0.02, seed=3)
    assert (inp["masks"].reshape(T, N)[1:] == 0).any(axis=1).mean() > 0.9   # nearly every step has an episode end somewhere
    held(f"accumulation {N} x {T}", *three_legs(L, inp, N, T))


def test_no_gradient_wanted(L):
    inp = {**GU.inputs("mix"), **U.affine(77)}
    layer = fused(L, U.layer_from(inp))
    full = run(layer, inp)
    c = lambda k, g=False: torch.tensor(inp[k], device="cuda", requires_grad=g)
    params = U.layer_params(layer)
    for p in params.values():
        p.grad = None
    x, h = c("x"), c("hxs", True)
    out, h_T = layer(x, h, c("masks"))
    ((out * c("g_out")).sum() + (h_T * c("g_h")).sum()).backward()
    assert x.grad is None
    np64 = lambda t: t.detach().double().cpu().numpy()
    got = {"out": np64(out), "h_T": np64(h_T).reshape(-1, U.H), "dhxs": np64(h.grad).reshape(-1, U.H), "dW_ih": np64(params["weight_ih_l0"].grad),
           "dW_hh": np64(params["weight_hh_l0"].grad), "db_ih": np64(params["bias_ih_l0"].grad), "db_hh": np64(params["bias_hh_l0"].grad),
           "dgamma": np64(params["norm.weight"].grad), "dbeta": np64(params["norm.bias"].grad)}
    for k, v in got.items():
        assert np.array_equal(v, full[k]), k
    # nothing requires grad: no graph, nothing returned for a backward
    for p in params.values():
        p.requires_grad_(False)
    out2, _ = layer(x, c("hxs"), c("masks"))
    assert not out2.requires_grad and np.array_equal(np64(out2), full["out"])
    for p in params.values():
        p.requires_grad_(True)
    with torch.no_grad():
        out3, h3 = layer(c("x", True), c("hxs", True), c("masks"))
    assert not out3.requires_grad and not h3.requires_grad
    assert np.array_equal(np64(out3), full["out"]) and np.array_equal(np64(h3).reshape(-1, U.H), full["h_T"])


def test_only_h_T_used(L):
    # no gradient reaches the LayerNorm: dgamma and dbeta are zero, everything else as the float64 restatement with g_out = 0
    inp = {**GU.inputs("mix"), **U.affine(78)}
    inp["g_out"] = np.zeros_like(inp["g_out"])
    N, T, _ = GU.CASES["mix"]
    layer = fused(L, U.layer_from(inp))
    c = lambda k, g=False: torch.tensor(inp[k], device="cuda", requires_grad=g)
    params = U.layer_params(layer)
    x, h = c("x", True), c("hxs", True)
    _, h_T = layer(x, h, c("masks"))
    (h_T * c("g_h")).sum().backward()
    assert not params["norm.weight"].grad.any() and not params["norm.bias"].grad.any()
    ref, f64 = run(U.layer_from(inp), inp), run_f64(inp, N, T)
    np64 = lambda t: t.detach().double().cpu().numpy()
    dev = {"dx": np64(x.grad), "dhxs": np64(h.grad).reshape(-1, U.H), "dW_ih": np64(params["weight_ih_l0"].grad), "dW_hh": np64(params["weight_hh_l0"].grad),
           "db_ih": np64(params["bias_ih_l0"].grad), "db_hh": np64(params["bias_hh_l0"].grad)}
    held("h_T alone", dev, ref, f64, keys=tuple(dev))


def test_determinism(L):
    inp = {**GU.inputs("mix"), **U.affine(79)}
    a = run(fused(L, U.layer_from(inp)), inp)
    b = run(fused(L, U.layer_from(inp)), inp)
    for k in U.KEYS:
        assert np.array_equal(a[k], b[k]), k


def test_side_stream(L):
    inp = {**GU.inputs("mix"), **U.affine(80)}
    layer = fused(L, U.layer_from(inp))
    base = run(layer, inp)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = run(layer, inp)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for k in U.KEYS:
        assert np.array_equal(base[k], side[k]), k


def test_no_host_synchronisation(L):
    inp = U.random_inputs(512, 60, seed=4)
    dev, ref = fused(L, U.layer_from(inp)), U.layer_from(inp)
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
    assert torch.isfinite(x.grad).all() and torch.isfinite(h.grad).all() and torch.isfinite(dev.norm.weight.grad).all()


def _flat(ts):
    return torch.cat([t.detach().double().reshape(-1) for t in ts]).cpu().numpy()


def test_whole_ppo_update(L, pkg):
    buf, nchunks, chunk = U.filled_buffer(pkg)
    sample = U.first_sample(buf, nchunks, chunk)
    assert all(isinstance(s, torch.Tensor) and s.is_cuda for s in sample)
    base = U.Policy(seed=11)
    runs = {}
    for kind in ("torch", "f64", "layer", "all"):
        pol, s = copy.deepcopy(base), sample
        adam_params = [p for grp in pol.optimizer.param_groups for p in grp["params"]]
        if kind == "f64":
            pol.actor.double(); pol.critic.double()
            s = tuple(t.double() for t in sample)
        if kind in ("layer", "all"):
            assert L.use_device_gru_layer(pol) == 2
            assert type(pol.actor.rnn) is L.DeviceFusedGRULayer and type(pol.critic.rnn) is L.DeviceFusedGRULayer
        if kind == "all":
            assert pkg.use_device_mlp(pol) == 4 and pkg.use_device_act(pol) == 1
            ret = pkg.DevicePPOTrainer(U.trainer_args(), torch.device("cuda", 0)).ppo_update(pol, sample)
            assert len(ret) == 6 and all(torch.isfinite(x).all() for x in ret)
        else:
            U.ppo_update(pol, s)
        params = list(pol.actor.parameters()) + list(pol.critic.parameters())
        # the optimiser built before the swap still holds the very Parameter objects the swapped modules use, and its state is on them
        assert [id(p) for p in adam_params] == [id(p) for p in params]
        assert all(p in pol.optimizer.state and "exp_avg" in pol.optimizer.state[p] for p in params)
        runs[kind] = (_flat([p.grad for p in params]), _flat(params))
    for kind in ("layer", "all"):
        for i, what in enumerate(("gradients", "parameters")):
            e_dev, e_ref = rel(runs[kind][i], runs["f64"][i]), rel(runs["torch"][i], runs["f64"][i])
            assert np.isfinite(runs[kind][i]).all()
            print(f"ppo update ({kind}) {what}: device {e_dev:.2e}, torch fp32 {e_ref:.2e}")
            assert e_dev <= max(4 * e_ref, FLOOR), (kind, what, e_dev, e_ref)
