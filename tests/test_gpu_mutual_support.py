"""The mutual-support discriminator on the MI355X (csrc/mutual_support.hpp, mutual_support.py): the scorer against float64 at the
smallest shapes that can break it, the gather against its host form, determinism, the rewards of a real collected rollout, training
against the reference's fixture and eager torch, and the stream discipline of intrinsic_rewards.

Bound (mutual_support_util.held): rel(device) <= max(4 * rel(torch fp32 eager on the same GPU), 2^-20) against float64 for the MSEs, and
the same factor times max|mse| for r_int, a difference with cancellation."""
import ctypes as C
import importlib
import types

import numpy as np
import pytest

import mutual_support_util as U

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def dptr(t):
    return None if t is None else t.data_ptr()


def device_score(pkg, w, a, E, na, s0, n, ratio=0.0, add=0):
    """ac_mi_score on device copies of the arrays: (mse, r_int, REWARDS after the call) as numpy."""
    lib = pkg.load_library()
    cu = lambda v: torch.tensor(np.ascontiguousarray(v, dtype=np.float32), device="cuda")
    da, dw = {k: cu(v) for k, v in a.items()}, {k: cu(v) for k, v in w.items()}
    mse = torch.full((n, E, 2, 2), float("nan"), device="cuda")
    r = torch.full((n, E, 2), float("nan"), device="cuda")
    args = U.score_struct(pkg, dw, da, E, na, s0, n, ratio, add, r, mse, ptr=dptr)
    assert lib.ac_mi_score(C.byref(args), torch.cuda.current_stream().cuda_stream) == 0, lib.last_error()
    torch.cuda.synchronize()
    return mse.cpu().numpy(), r.cpu().numpy(), da["REWARDS"].cpu().numpy()


# The row tile is 128 rows = 64 (step, env) pairs; 256 workgroups at most, so more than 16384 pairs make a workgroup walk a second tile.
SHAPES = [  # (T, E, na, D, C, s0, n)
    (1, 1, 2, 39, 7, 0, 1),          # one pair
    (4, 5, 2, 15, 1, 1, 3),          # 15 pairs: a partial tile; s0 > 0
    (2, 63, 2, 16, 12, 1, 1),        # one pair less than the tile
    (1, 64, 4, 17, 7, 0, 1),         # the tile exactly
    (3, 65, 2, 1, 7, 2, 1),          # one pair more
    (4, 45, 4, 65, 12, 1, 3),        # 135 pairs: two tiles and a remainder; steps and envs both cross tiles
    (2, 9, 2, 128, 1, 0, 2),         # the widest observation
    (8, 2100, 2, 39, 7, 0, 8),       # 16800 pairs: the persistent loop's second pass
]


@pytest.mark.parametrize("T,E,na,D,C_,s0,n", SHAPES)
def test_scorer_against_float64(pkg, T, E, na, D, C_, s0, n):
    a, w = U.arrays(T, E, na, D, C_), U.weights(D, C_, seed=3)
    mse, r, rew = device_score(pkg, w, a, E, na, s0, n)
    assert np.isfinite(mse).all() and np.isfinite(r).all()
    assert np.array_equal(rew, a["REWARDS"])
    U.held(f"device {(T, E, na, D, C_, s0, n)}", mse, r, w, a, s0, n, E, na, device="cuda")


def test_two_runs_are_bit_identical_and_add_is_exact(pkg):
    T, E, na, D, C_, s0, n = 4, 45, 4, 65, 12, 1, 3
    a, w = U.arrays(T, E, na, D, C_), U.weights(D, C_, seed=3)
    ratio = np.float32(0.37)
    m1, r1, rew1 = device_score(pkg, w, a, E, na, s0, n, ratio=float(ratio), add=1)
    m2, r2, rew2 = device_score(pkg, w, a, E, na, s0, n, ratio=float(ratio), add=1)
    assert np.array_equal(m1, m2) and np.array_equal(r1, r2) and np.array_equal(rew1, rew2)
    want = a["REWARDS"].copy().reshape(T, E, na)
    want[s0:s0 + n, :, :2] += ratio * r1
    assert np.array_equal(rew1.reshape(T, E, na), want)       # once, to agents 0 and 1 of the steps asked for, and nothing else
    big = (8, 2100, 2, 39, 7, 0, 8)
    a, w = U.arrays(*big[:5]), U.weights(39, 7, seed=3)
    x, y = device_score(pkg, w, a, 2100, 2, 0, 8), device_score(pkg, w, a, 2100, 2, 0, 8)
    assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


@pytest.mark.parametrize("T,E,na,D,C_,times", [
    (5, 3, 2, 39, 7, [4, 0]),
    (4, 2, 4, 15, 7, [3, 1, 2]),
    (3, 1, 2, 1, 1, [2]),
    (6, 70, 3, 128, 12, [0, 5, 5, 1]),
])
def test_device_gather_equals_host_gather(pkg, T, E, na, D, C_, times):
    lib = pkg.load_library()
    a = U.arrays(T, E, na, D, C_)
    hX, hY = U.host_gather(pkg, a, E, na, times)
    da = {k: torch.tensor(v, device="cuda") for k, v in a.items()}
    t = torch.tensor(times, dtype=torch.int32, device="cuda")
    X, Y = torch.full(hX.shape, float("nan"), device="cuda"), torch.full(hY.shape, float("nan"), device="cuda")
    args = U.gather_struct(pkg, da, E, na, t, X, Y, ptr=dptr)
    assert lib.ac_mi_gather(C.byref(args), torch.cuda.current_stream().cuda_stream) == 0, lib.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(X.cpu().numpy(), hX) and np.array_equal(Y.cpu().numpy(), hY)


def buffer_args(T, E, **kw):
    d = dict(buffer_size=T, n_rollout_threads=E, gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False,
             recurrent_hidden_size=128, recurrent_hidden_layers=1)
    d.update(kw)
    return types.SimpleNamespace(**d)


def filled_buffer(pkg, a, T, E, na, D, C_):
    """A DeviceSharedReplayBuffer holding the arrays of mutual_support_util.arrays."""
    buf = pkg.DeviceSharedReplayBuffer(buffer_args(T, E), na, D, na * D, U.Space(shape=(C_,), nvec=np.full(C_, 41)))
    for t in range(T + 1):
        buf.set_slot("obs", t, a["OBS"][t].reshape(E, na, D))
        buf.set_slot("rnn_states_actor", t, a["RNN_ACTOR"][t].reshape(E, na, 1, U.H))
    for t in range(T):
        buf.set_slot("actions", t, a["ACTIONS"][t].reshape(E, na, C_))
        buf.set_slot("rewards", t, a["REWARDS"][t].reshape(E, na, 1))
    return buf


def cuda_disc(pkg, D, C_, num_agents=2, w=None, **kw):
    disc = pkg.DeviceDiscriminator(U.disc_args(**kw), num_agents, *U.spaces(D, C_), device=torch.device("cuda", 0))
    if w is not None:
        disc.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return disc


def test_intrinsic_rewards_of_a_filled_buffer(pkg):
    """The Python path on known contents: r_int [n, E, na, 1] with agents >= 2 exactly 0, the default ratio and range, add=False."""
    T, E, na, D, C_ = 4, 7, 3, 15, 7
    a, w = U.arrays(T, E, na, D, C_), U.weights(D, C_)
    buf, disc = filled_buffer(pkg, a, T, E, na, D, C_), cuda_disc(pkg, D, C_, num_agents=na, w=w, intrinsic_ratio=0.25)
    r = disc.intrinsic_rewards(buf, add=False)
    mse = disc.step_mse(buf)
    torch.cuda.synchronize()
    assert r.shape == (T, E, na, 1) and not r[:, :, 2:].any()
    assert np.array_equal(buf.array("rewards").reshape(T, E * na), a["REWARDS"])
    U.held("filled buffer", mse.cpu().numpy(), r[:, :, :2, 0].cpu().numpy(), w, a, 0, T, E, na, device="cuda")
    r2 = disc.intrinsic_rewards(buf, start=1, n_steps=2)          # add=True, ratio = args.intrinsic_ratio
    torch.cuda.synchronize()
    assert torch.equal(r2, r[1:3])
    want = a["REWARDS"].copy().reshape(T, E, na)
    want[1:3] += np.float32(0.25) * r2[..., 0].cpu().numpy()
    assert np.array_equal(buf.array("rewards").reshape(T, E, na), want)
    with pytest.raises(ValueError, match="DeviceSharedReplayBuffer is needed"):
        disc.intrinsic_rewards(pkg.DeviceReplayBuffer(buffer_args(T, E), na, D, U.Space(shape=(C_,), nvec=np.full(C_, 41))))
    with pytest.raises(ValueError, match=r"are not inside the buffer's \[0, 4\)"):
        disc.intrinsic_rewards(buf, start=3, n_steps=2)
    assert np.array_equal(buf.array("rewards").reshape(T, E, na), want)     # a refusal touches nothing


def test_intrinsic_rewards_after_a_real_collect(pkg):
    """After DeviceMAPPORollout.collect on a small 2v2 env (all four aircraft the learner's: na = 4) the rewards gain ratio * r_int of
    the buffer's own slots, as the host row function computes it, and no other field of the buffer changes."""
    RS = importlib.import_module("test_gpu_rollout_share")
    P = importlib.import_module("aircombat-selfplay_amd.policy")
    side = RS.Side(pkg, P, "mc_all")
    buf, E, T, na = side.buffer, RS.E, RS.T, side.na
    side.rollout().collect()
    torch.cuda.synchronize()
    before = {k: buf.array(k) for k in RS.FIELDS}
    D, C_ = side.D, int(np.prod(buf.act_shape))
    w = U.weights(D, C_, seed=4)
    disc = pkg.DeviceDiscriminator(U.disc_args(intrinsic_ratio=0.5), na, side.env.observation_space, side.env.share_observation_space,
                                   side.env.action_space, device=torch.device("cuda", 0))
    assert (disc.act_dim, disc.output_dim) == (C_, D)
    disc.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    r = disc.intrinsic_rewards(buf)
    torch.cuda.synchronize()
    after = {k: buf.array(k) for k in RS.FIELDS}
    for k in RS.FIELDS:
        if k != "rewards":
            assert np.array_equal(before[k], after[k]), k
    r = r.cpu().numpy()
    assert r.shape == (T, E, na, 1) and not r[:, :, 2:].any() and np.abs(r).max() > 0
    assert np.array_equal(after["rewards"], before["rewards"] + np.float32(0.5) * r)
    a = {"OBS": before["obs"].reshape(T + 1, E * na, D), "ACTIONS": before["actions"].reshape(T, E * na, C_),
         "RNN_ACTOR": before["rnn_states_actor"].reshape(T + 1, E * na, U.H), "REWARDS": before["rewards"].reshape(T, E * na)}
    assert np.abs(a["RNN_ACTOR"][1:]).max() > 0 and np.abs(a["ACTIONS"]).max() > 0        # a real rollout: states and actions are live
    h_mse, h_r, h_rew = U.host_score(pkg, w, a, E, na, 0, T, ratio=0.5, add=1)
    ref_mse, ref_r = U.score(w, a, 0, T, E, na, torch.float64)
    t32_mse, _ = U.score(w, a, 0, T, E, na, torch.float32, "cuda")
    factor = max(4.0 * U.rel(t32_mse, ref_mse), 2.0 ** -20)
    scale = np.abs(ref_mse).max()
    print(f"collect: device-f64 {np.abs(r[:, :, :2, 0] - ref_r).max():.3e}  host-f64 {np.abs(h_r - ref_r).max():.3e}  allowed {factor * scale:.3e}")
    assert np.abs(r[:, :, :2, 0] - ref_r).max() <= factor * scale and np.abs(h_r - ref_r).max() <= factor * scale
    # and the rewards themselves against the host row function's: each side's r_int is within the bound of float64
    assert np.abs(after["rewards"].reshape(T, E * na) - h_rew).max() <= 0.5 * 2 * factor * scale + 2.0 ** -23 * np.abs(h_rew).max()


def test_no_host_synchronisation_in_intrinsic_rewards(pkg):
    T, E, na, D, C_ = 4, 70, 4, 39, 7
    a, w = U.arrays(T, E, na, D, C_), U.weights(D, C_)
    buf, disc = filled_buffer(pkg, a, T, E, na, D, C_), cuda_disc(pkg, D, C_, num_agents=na, w=w)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r = disc.intrinsic_rewards(buf, ratio=0.1)
        m = disc.step_mse(buf)
        with pytest.raises(RuntimeError):      # the check is live: a read on the host is refused
            r.sum().item()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(r).all() and torch.isfinite(m).all()


def test_train_against_the_reference_and_eager_torch(pkg):
    """Two epochs of two mini-batches with the fixture's time orders: the four losses and the trained weights against the reference's
    float64 run (tests/golden/mutual_support.npz), the comparator being eager torch fp32 doing the same steps on this GPU (indexing,
    cat, the Linears, mse_loss, torch's Adam). The weights are held as ONE vector of all twelve tensors, as the whole-update tests of
    the training layers hold theirs: a bias of 39 values alone has too few entries for its eager error to be a yardstick."""
    g, t = np.load(U.GOLDEN), U.TRAIN
    T, E, na, D, C_ = t["T"], t["E"], t["na"], t["D"], t["C"]
    a, w = U.arrays(T, E, na, D, C_), U.weights(D, C_)
    buf = filled_buffer(pkg, a, T, E, na, D, C_)
    disc = cuda_disc(pkg, D, C_, w=w, ppo_epoch=t["ppo_epoch"], num_mini_batch=t["num_mini_batch"], lr=t["lr"])
    info = disc.train(buf, time_orders=U.TRAIN_ORDERS)
    dev_losses = disc.last_losses.double().cpu().numpy()
    assert set(info) == {"disc_loss"} and abs(info["disc_loss"] - dev_losses.mean()) <= 1e-6 * dev_losses.mean()
    for k in ("obs", "actions", "rnn_states_actor", "rewards"):      # training reads the buffer and writes nothing
        assert np.array_equal(buf.array(k).reshape(-1), a[{"obs": "OBS", "actions": "ACTIONS", "rnn_states_actor": "RNN_ACTOR", "rewards": "REWARDS"}[k]].reshape(-1)), k
    # eager torch fp32, the same steps
    ew = {k: torch.tensor(v, device="cuda", requires_grad=True) for k, v in w.items()}
    ea = {k: torch.tensor(v, device="cuda") for k, v in a.items()}
    opt = torch.optim.Adam([ew[k] for k in U.KEYS], lr=t["lr"])
    mb, eager_losses = T // t["num_mini_batch"], []
    for order in U.TRAIN_ORDERS:
        for i in range(t["num_mini_batch"]):
            X, Y = U.tuples(ea, order[i * mb:(i + 1) * mb], E, na)
            half = X.shape[0] // 2
            p, q = U.mlp(ew, "pred", X), U.mlp(ew, "pred_wo", X[:, :U.H + C_])
            loss = 0.01 * sum(torch.nn.functional.mse_loss(o[rows], Y[rows]) for rows in (slice(0, half), slice(half, None)) for o in (p, q))
            opt.zero_grad()
            loss.backward()
            opt.step()
            eager_losses.append(float(loss.detach()))
    flat = lambda d: np.concatenate([np.asarray(d[k], dtype=np.float64).reshape(-1) for k in U.KEYS])
    ref_losses = g["train/losses"]
    ref_w = flat({k: w[k].astype(np.float64) + g["train/delta/" + k].astype(np.float64) for k in U.KEYS})
    dev_w = flat({k: v.detach().cpu().numpy() for k, v in disc.state_dict().items()})
    eag_w = flat({k: v.detach().cpu().numpy() for k, v in ew.items()})
    assert np.abs(dev_w - flat(w)).max() > 1e-3                      # training moved the weights
    for what, dev, eager, ref in (("losses", dev_losses, eager_losses, ref_losses), ("weights", dev_w, eag_w, ref_w)):
        e_dev, e_eager = U.rel(dev, ref), U.rel(eager, ref)
        print(f"train {what}: device {e_dev:.3e}, torch fp32 {e_eager:.3e}")
        assert e_dev <= max(4.0 * e_eager, 2.0 ** -20), (what, e_dev, e_eager)
    # the default orders come from the device generator and the call runs as well
    assert np.isfinite(disc.train(buf)["disc_loss"])
