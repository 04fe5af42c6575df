"""The mutual-support discriminator without a GPU (include/aircombat_mutual.h, csrc/mutual_support.hpp, mutual_support.py): the exports,
the checkpoint's key names, the gather's and the scorer's host row functions against indexing, the reference's compute_MI fixture and a
float64 restatement, what `add` touches, and every refusal."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import mutual_support_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ac_mi_score", "ac_mi_score_host", "ac_mi_gather", "ac_mi_gather_host")


@pytest.fixture(scope="module")
def golden():
    return np.load(U.GOLDEN)


def cpu_disc(pkg, D=39, C_=7, num_agents=2, **kw):
    return pkg.DeviceDiscriminator(U.disc_args(**kw), num_agents, *U.spaces(D, C_), device=torch.device("cpu"))


def test_exports_and_symbols(pkg, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "aircombat_mutual.h")).read()
    assert set(re.findall(r"\b(ac_mi_[a-z0-9_]+)\s*\(", hdr)) == set(SYMBOLS)
    lib = pkg.load_library()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib.path], text=True)
    for sym in SYMBOLS:
        assert sym in pkg.capi.SIGNATURES and hasattr(lib, sym) and re.search(rf"\bT {sym}\b", exported), sym
    assert "DeviceDiscriminator" in pkg.__all__ and pkg.DeviceDiscriminator.__name__ == "DeviceDiscriminator"
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "aircombat_mutual.h"\n'
                   'int main(){printf("%zu %zu", sizeof(ac_mi_score_t), sizeof(ac_mi_gather_t));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    a, b = map(int, subprocess.check_output([str(tmp_path / "sz")], text=True).split())
    assert (a, b) == (C.sizeof(pkg.capi.AcMiScore), C.sizeof(pkg.capi.AcMiGather))


def test_package_imports_without_torch():
    code = ("import sys, aircombat_selfplay_amd as p; assert 'torch' not in sys.modules; "
            "assert 'DeviceDiscriminator' in p.__all__ and 'DeviceDiscriminator' in p._TORCH_EXPORTS; print('ok')")
    assert subprocess.check_output([sys.executable, "-c", code], cwd=ROOT, text=True).strip() == "ok"


def test_state_dict_keys_are_the_checkpoints(pkg, golden):
    disc = cpu_disc(pkg)
    assert list(disc.state_dict()) == [str(k) for k in golden["keys"]] == U.KEYS
    assert disc.pred.layers[0].weight.shape == (256, 142) and disc.pred_wo.layers[0].weight.shape == (256, 135)
    assert disc.pred.last_fc.weight.shape == (39, 256) and disc.q_loss_coef == 0.01
    opt = disc.q_optimizer
    assert isinstance(opt, torch.optim.Adam) and len(opt.param_groups) == 1 and opt.param_groups[0]["lr"] == 1e-3
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in list(disc.pred.parameters()) + list(disc.pred_wo.parameters())]
    disc.load_state_dict({k: torch.from_numpy(v) for k, v in U.weights(39, 7).items()})     # a reference checkpoint loads
    assert disc.eval() is disc and not disc.training and disc.train(True).training           # nn.Module's own train(mode) is kept


@pytest.mark.parametrize("T,E,na,D,C_,times", [
    (5, 3, 2, 39, 7, [4, 0]),              # m does not divide T; the last slot T - 1 -> T
    (4, 2, 4, 15, 7, [3, 1, 2]),           # four agents: rows of agents 2, 3 are never read
    (3, 1, 2, 1, 1, [2]),
    (6, 5, 3, 128, 12, [0, 5, 5, 1]),      # a repeated index
])
def test_gather_host_equals_indexing(pkg, T, E, na, D, C_, times):
    a = U.arrays(T, E, na, D, C_)
    X, Y = U.host_gather(pkg, a, E, na, times)
    wantX, wantY = U.tuples(a, times, E, na)
    assert X.shape == wantX.shape and Y.shape == wantY.shape
    assert np.array_equal(X, wantX) and np.array_equal(Y, wantY)


@pytest.mark.parametrize("D,C_", U.MI_CASES)
def test_score_host_against_the_reference_compute_MI(pkg, golden, D, C_):
    a, w = U.mi_as_buffer(D, C_), U.weights(D, C_)
    for k, v in zip(("h", "actions", "next_obs"), U.mi_inputs(D, C_)):
        assert np.array_equal(golden[f"mi/{D}_{C_}/{k}"], v), k        # the fixture's inputs are the regenerated ones
    ref = golden[f"mi/{D}_{C_}/out"]                                    # [64, agent]
    mse, r, _ = U.host_score(pkg, w, a, 64, 2, 0, 1)
    ref_mse, ref_r = U.score(w, a, 0, 1, 64, 2, torch.float64)
    # the float64 restatement IS the reference's compute_MI, which rounds its result once into a float32 array
    assert (np.abs(ref_r[0] - ref) <= 2.0 ** -24 * np.abs(ref) + 1e-13).all()
    U.held(f"host D={D}", mse, r, w, a, 0, 1, 64, 2)
    # and the module's own compute_MI, plain torch fp32
    disc = cpu_disc(pkg, D, C_)
    disc.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    h, act, nxt = U.mi_inputs(D, C_)
    got = np.stack([disc.compute_MI(np.zeros((2, D)), nxt[i], act[i], np.zeros((2, 1)), h[i].reshape(1, 1, U.H)) for i in range(8)])
    assert got.shape == (8, 2) and np.abs(got - ref[:8]).max() <= 64 * 2.0 ** -23 * np.abs(ref_mse).max()


EDGES = [  # (T, E, na, D, C, s0, n)
    (1, 1, 2, 1, 1, 0, 1),
    (3, 5, 2, 15, 7, 0, 3),
    (3, 2, 4, 16, 12, 1, 2),
    (2, 3, 3, 17, 1, 1, 1),
    (2, 2, 2, 65, 7, 0, 2),
    (2, 1, 2, 128, 12, 0, 2),
]


@pytest.mark.parametrize("T,E,na,D,C_,s0,n", EDGES)
def test_score_host_against_float64(pkg, T, E, na, D, C_, s0, n):
    a, w = U.arrays(T, E, na, D, C_), U.weights(D, C_, seed=2)
    mse, r, rew = U.host_score(pkg, w, a, E, na, s0, n)
    assert np.array_equal(rew, a["REWARDS"])            # add = 0: untouched
    U.held(f"host {(T, E, na, D, C_, s0, n)}", mse, r, w, a, s0, n, E, na)


def test_add_adds_ratio_times_r_int_once_and_nothing_else(pkg):
    T, E, na, D, C_, s0, n = 4, 3, 4, 15, 7, 1, 2
    a, w = U.arrays(T, E, na, D, C_), U.weights(D, C_)
    ratio = np.float32(0.37)
    _, r, rew = U.host_score(pkg, w, a, E, na, s0, n, ratio=float(ratio), add=1)
    want = a["REWARDS"].copy().reshape(T, E, na)
    want[s0:s0 + n, :, :2] += ratio * r                 # float32 throughout, as the row function
    assert np.array_equal(rew.reshape(T, E, na), want)
    assert np.array_equal(rew.reshape(T, E, na)[:, :, 2:], a["REWARDS"].reshape(T, E, na)[:, :, 2:])     # agents >= 2: exactly 0 added
    assert not np.array_equal(rew, a["REWARDS"])
    _, r0, rew0 = U.host_score(pkg, w, a, E, na, s0, n, ratio=float(ratio), add=0)
    assert np.array_equal(r0, r) and np.array_equal(rew0, a["REWARDS"])


def test_c_abi_refusals_name_the_value(pkg):
    lib = pkg.load_library()
    a, w = U.arrays(2, 2, 2, 15, 7), {k: np.ascontiguousarray(v) for k, v in U.weights(15, 7).items()}
    r = np.zeros((2, 2, 2), np.float32)
    for over, msg in [(dict(act_dim=0), "act_dim 0"), (dict(act_dim=13), "act_dim 13"), (dict(obs_dim=0), "obs_dim 0"), (dict(obs_dim=129), "obs_dim 129"),
                      (dict(hidden=64), "hidden 64"), (dict(na=1), "na 1"), (dict(E=0), "E 0"), (dict(s0=-1), "s0 -1"), (dict(n=0), "n 0"),
                      (dict(s0=1, n=2), "s0 + n = 3 exceeds T = 2"), (dict(OBS=None), "null"), (dict(add=1, REWARDS=None), "REWARDS is NULL")]:
        args = U.score_struct(pkg, w, a, 2, 2, 0, 2, r_int=r, over=over)
        assert lib.ac_mi_score_host(C.byref(args)) == -1 and msg in lib.last_error(), (over, lib.last_error())
        assert lib.ac_mi_score(C.byref(args), None) == -1 and msg in lib.last_error(), (over, lib.last_error())    # refused before any launch
    assert not r.any()
    times = np.array([0, 1], np.int32)
    X, Y = np.zeros((8, 142), np.float32), np.zeros((8, 15), np.float32)
    for over, msg in [(dict(m=0), "m 0"), (dict(act_dim=13), "act_dim 13"), (dict(obs_dim=200), "obs_dim 200"), (dict(na=1), "na 1"),
                      (dict(hidden=256), "hidden 256"), (dict(X=None), "null")]:
        args = U.gather_struct(pkg, a, 2, 2, times, X, Y, over=over)
        assert lib.ac_mi_gather_host(C.byref(args)) == -1 and msg in lib.last_error(), (over, lib.last_error())
        assert lib.ac_mi_gather(C.byref(args), None) == -1 and msg in lib.last_error(), (over, lib.last_error())
    for bad in (2, -1):
        args = U.gather_struct(pkg, a, 2, 2, np.array([0, bad], np.int32), X, Y)
        assert lib.ac_mi_gather_host(C.byref(args)) == -1 and f"time index {bad}" in lib.last_error()
    assert not X.any() and not Y.any()


def shell_buffer(pkg, cls, device_id=0, num_agents=2, D=39, C_=7, T=8, E=3, hidden=128, layers=1):
    """A buffer object with the attributes the checks read and no handle: a refusal must come before anything is touched."""
    b = object.__new__(cls)
    b.device_id, b.num_agents, b.obs_shape, b.act_shape = device_id, num_agents, (D,), (C_,)
    b.buffer_size, b.n_rollout_threads, b.recurrent_hidden_size, b.recurrent_hidden_layers = T, E, hidden, layers
    return b


def test_python_refusals(pkg):
    with pytest.raises(ValueError, match="num_agents 1"):
        cpu_disc(pkg, num_agents=1)
    for kw, msg in [(dict(hidden_size="64 64"), "64 64"), (dict(hidden_size="128"), "'128'"), (dict(recurrent_hidden_size=64), "64")]:
        with pytest.raises(pkg.UnsupportedPolicy, match=msg):
            cpu_disc(pkg, **kw)
    with pytest.raises(pkg.UnsupportedPolicy, match="13 action columns"):
        cpu_disc(pkg, C_=13)
    with pytest.raises(pkg.UnsupportedPolicy, match="obs_dim 129"):
        cpu_disc(pkg, D=129)
    disc = cpu_disc(pkg)
    S, P = pkg.DeviceSharedReplayBuffer, pkg.DeviceReplayBuffer
    for method in (disc.intrinsic_rewards, disc.train, disc.step_mse):
        with pytest.raises(ValueError, match="DeviceSharedReplayBuffer is needed, got DeviceReplayBuffer"):
            method(shell_buffer(pkg, P))
        with pytest.raises(ValueError, match="the buffer is on cuda:0, the discriminator on cpu"):
            method(shell_buffer(pkg, S))
    disc.device = torch.device("cuda", 0)         # only the checks run below: they end before any parameter or array is touched
    with pytest.raises(ValueError, match="the buffer is on cuda:1"):
        disc.intrinsic_rewards(shell_buffer(pkg, S, device_id=1))
    with pytest.raises(ValueError, match="1 agent"):
        disc.intrinsic_rewards(shell_buffer(pkg, S, num_agents=1))
    for kw in (dict(num_agents=4), dict(D=40), dict(C_=6), dict(hidden=64), dict(layers=2)):
        with pytest.raises(ValueError, match="the discriminator's are"):
            disc.intrinsic_rewards(shell_buffer(pkg, S, **kw))
    for start, n in ((0, 9), (8, 1), (-1, 2), (3, 0), (5, 4)):
        with pytest.raises(ValueError, match=r"are not inside the buffer's \[0, 8\)"):
            disc.intrinsic_rewards(shell_buffer(pkg, S), start=start, n_steps=n)
    with pytest.raises(ValueError, match="do not fill"):
        disc.num_mini_batch = 9
        disc.train(shell_buffer(pkg, S))
    disc.num_mini_batch = 2
    with pytest.raises(ValueError, match="must be contiguous float32 on cuda:0"):     # the CPU parameters themselves
        disc.intrinsic_rewards(shell_buffer(pkg, S))
