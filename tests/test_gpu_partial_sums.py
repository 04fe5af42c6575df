"""The order in which the training layers' parameter gradients are summed (trn::sum_sets of csrc/train_common.hpp, called by
mlp_block_reduce, act_eval_reduce and gru_sum_partials), on the MI355X: "an order fixed by the number of sets alone".

Each backward C entry point is called with a workspace of the test's own. The workspace is read back and its sets are added in numpy
float32 in the documented order: chain j takes sets j, j + 8, .. ascending from 0, then ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)).
The gradients the call returned must equal that bit for bit. The shapes are the smallest at which the order can go wrong: one set, eleven
sets (one full round of the eight chains and a tail of three) and the cap on the number of sets. Inputs are standard normal, so no
partial sum is subnormal and the device's flush-to-zero cannot differ from numpy.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
H = 128


def documented_sum(ws, S, nel):
    sets = ws[:S * nel].reshape(S, nel)
    a = np.zeros((8, nel), np.float32)
    for s in range(S):
        a[s % 8] += sets[s]
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))


def same_bits(what, got, want):
    got, want = got.detach().cpu().numpy().ravel(), np.asarray(want, np.float32).ravel()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(want).all() and np.abs(want).max() > 0, what
    differ = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert differ.size == 0, (what, differ.size, got[differ[:4]], want[differ[:4]])


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def normal(gen, *shape):
    return torch.randn(*shape, generator=gen, device="cuda", dtype=torch.float32)


def launch(lib, name, *args):
    stream = torch.cuda.current_stream().cuda_stream
    rc = getattr(lib, name)(0, stream, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])
    assert rc == 0, (name, lib.last_error())


def workspace(lib, name, *args):
    floats = getattr(lib, name)(*args)
    assert floats > 0, (name, lib.last_error())
    return torch.zeros(floats, device="cuda", dtype=torch.float32)


M_CASES = ((1, 1), (352, 11), (8224, 256))   # rows, partial sets: 32-row tiles, 256 sets at most (257 tiles here)


@pytest.mark.parametrize("K", [7, 256])
@pytest.mark.parametrize("M,sets", M_CASES)
def test_mlp_block_backward(lib, M, sets, K):
    gen = torch.Generator(device="cuda").manual_seed(1000 * K + M)
    x, w, b, gamma, beta, dy = normal(gen, M, K), normal(gen, H, K), normal(gen, H), normal(gen, H), normal(gen, H), normal(gen, M, H)
    y, stats = torch.empty(M, H, device="cuda"), torch.empty(M, 2, device="cuda")
    launch(lib, "ac_mlp_block_forward", M, K, 1e-5, x, w, b, gamma, beta, y, stats)
    nel = H * K + 3 * H
    ws = workspace(lib, "ac_mlp_block_workspace_floats", M, K)
    assert ws.numel() == sets * nel
    dx, dw, db, dgamma, dbeta = (torch.empty(s, device="cuda") for s in ((M, K), (H, K), (H,), (H,), (H,)))
    launch(lib, "ac_mlp_block_backward", M, K, dy, x, w, b, gamma, stats, ws, dx, dw, db, dgamma, dbeta)
    torch.cuda.synchronize()
    want = documented_sum(ws.cpu().numpy(), sets, nel)
    same_bits("dW, db, dgamma, dbeta", torch.cat([dw.ravel(), db, dgamma, dbeta]), want)


@pytest.mark.parametrize("M,sets", M_CASES)
def test_act_eval_backward(lib, pkg, M, sets):
    nvec, shoot_cols = (3, 5, 3), 4
    sizes = nvec + (2,)                      # the categorical heads, then the one shoot head that takes part
    total = sum(sizes)
    gen = torch.Generator(device="cuda").manual_seed(M)
    heads = pkg.capi.AcActHeads(n_cat=len(nvec), n_shoot_cols=shoot_cols)
    heads.nvec[:len(nvec)] = list(nvec)
    x, dlogp, dent = normal(gen, M, H), normal(gen, M), normal(gen, M)
    ws_, bs = [normal(gen, n, H) for n in sizes], [normal(gen, n) for n in sizes]
    cols = [torch.randint(0, n, (M, 1), generator=gen, device="cuda") for n in nvec + (2,) * shoot_cols]
    action = torch.cat(cols, 1).to(torch.float32).contiguous()
    alpha0, beta0 = (1.0 + 2.0 * torch.rand(M, generator=gen, device="cuda") for _ in range(2))
    dws, dbs = [torch.empty_like(t) for t in ws_], [torch.empty_like(t) for t in bs]
    ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    nel = (H + 1) * total
    ws = workspace(lib, "ac_act_eval_workspace_floats", C.byref(heads), M)
    assert ws.numel() == sets * nel
    dx = torch.empty(M, H, device="cuda")
    launch(lib, "ac_act_eval_backward", C.byref(heads), M, dlogp, dent, x, ptrs(ws_), ptrs(bs), action, alpha0, beta0, ws, dx, ptrs(dws),
           ptrs(dbs))
    torch.cuda.synchronize()
    want = documented_sum(ws.cpu().numpy(), sets, nel)   # a set: the stacked dW [total, 128], then the stacked db [total]
    same_bits("dW, db of every head", torch.cat([t.ravel() for t in dws] + dbs), want)


@pytest.mark.parametrize("N,T,tiles", [(1, 1, 1), (176, 2, 11), (4128, 1, 129)])
def test_gru_layer_backward(lib, N, T, tiles):
    rt, ln_cap, dw_cap = (lib.ac_gru_layer_constant(i) for i in (0, 3, 4))
    M = N * T
    assert (rt, dw_cap) == (32, 128) and tiles == (M + rt - 1) // rt
    dw_sets, ln_sets = min(tiles, dw_cap), min(tiles, ln_cap)
    gen = torch.Generator(device="cuda").manual_seed(M)
    x, hxs, g_out, g_h = normal(gen, M, H), normal(gen, N, H), normal(gen, M, H), normal(gen, N, H)
    masks = (torch.rand(M, generator=gen, device="cuda") > 0.1).to(torch.float32)
    w_ih, w_hh, b_ih, b_hh = normal(gen, 3 * H, H), normal(gen, 3 * H, H), normal(gen, 3 * H), normal(gen, 3 * H)
    w_ih, w_hh = w_ih / 8, w_hh / 8          # gates that do not all saturate
    gamma, beta = normal(gen, H), normal(gen, H)
    new = lambda *s: torch.empty(*s, device="cuda", dtype=torch.float32)
    out, h_T, y, saved, stats = new(M, H), new(N, H), new(M, H), new(M, 4 * H), new(M, 2)
    launch(lib, "ac_gru_layer_forward", N, T, x, hxs, masks, w_ih, w_hh, b_ih, b_hh, gamma, beta, 1e-5, new(M * 3 * H), out, h_T, y, saved,
           stats)
    # the backward's workspace: [dgi: M * 384][dgh: M * 384][dy: M * 128][gru_dw's sets, dW_ih's then dW_hh's][gru_ln_bwd's sets]
    dw_nel, ln_nel = 3 * H * H + 3 * H, 2 * H
    dwp = 2 * M * 3 * H + M * H
    lnp = dwp + 2 * dw_sets * dw_nel
    ws = workspace(lib, "ac_gru_layer_workspace_floats", N, T)
    assert ws.numel() == lnp + ln_sets * ln_nel
    dx, dhxs, dw_ih, dw_hh, db_ih, db_hh, dgamma, dbeta = new(M, H), new(N, H), new(3 * H, H), new(3 * H, H), new(3 * H), new(3 * H), new(H), new(H)
    launch(lib, "ac_gru_layer_backward", N, T, g_out, g_h, x, hxs, masks, w_ih, w_hh, gamma, y, saved, stats, ws, dx, dhxs, dw_ih, dw_hh,
           db_ih, db_hh, dgamma, dbeta)
    torch.cuda.synchronize()
    host = ws.cpu().numpy()
    same_bits("dW_ih, db_ih", torch.cat([dw_ih.ravel(), db_ih]), documented_sum(host[dwp:], dw_sets, dw_nel))
    same_bits("dW_hh, db_hh", torch.cat([dw_hh.ravel(), db_hh]), documented_sum(host[dwp + dw_sets * dw_nel:], dw_sets, dw_nel))
    same_bits("dgamma, dbeta", torch.cat([dgamma, dbeta]), documented_sum(host[lnp:], ln_sets, ln_nel))
