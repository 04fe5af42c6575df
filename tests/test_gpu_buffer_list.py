"""The list form of the device buffers on the MI355X (include/aircombat_epoch.h, ac_buffers_*; csrc/epoch_gather_multi.hpp;
DeviceReplayBuffer.recurrent_generator([...]), epoch_of, DevicePPOTrainer.train(policy, [...])).

The gather is a copy, so every gathered field is compared bit for bit: against the golden vectors from the reference's own
``ReplayBuffer.recurrent_generator([b0, ...])`` (tests/golden/buffer_list.npz) and, for the shapes the golden does not hold, against the
numpy restatement that tests/test_buffer_list_host.py holds to that golden. The one field with arithmetic is the advantages: each
buffer's own, normalised by fp64 block sums where numpy sums pairwise in float32, held to tests/test_rollout_buffer.py's bound
|d| <= 2e-6 + 2e-6 |x|; where a restatement is given the device's advantages they, too, must come back bit for bit.

Shapes: the golden's two cases (a chunk across two buffers on the scalar path; agents, column straddles, the 16-byte path, a dropped
remainder); K = 1 and K = 8; 160 step rows and 80 state rows (past the kernel's 64-row tile, no multiple of it); a shared pair.
Out-of-range indices reach the device only in the clamp test, where the kernel's clamp is what is tested."""
import copy
import ctypes as C
import importlib
import os
import types

import numpy as np
import pytest

import act_train_util as AU
import buffer_list_util as U
import ppo_update_util as PU

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "buffer_list.npz")
FLOOR = 2.0 ** -20

K8 = dict(K=8, T=4, E=2, A=1, L=3, n_mb=2, obs=5, act=2, hidden=4, seed=303)         # 64 rows, 21 chunks across 8 buffers
TILES = dict(K=2, T=16, E=5, A=1, L=2, n_mb=2, obs=8, act=4, hidden=4, seed=404)      # 80 chunks: 160 step rows, 80 state rows
SHARED = dict(K=2, T=5, E=2, A=2, L=3, n_mb=2, obs=8, act=4, hidden=4, seed=505)      # share_obs of 16 floats


def golden():
    return np.load(GOLDEN)


def device_buffers(pkg, case, share=0):
    out = []
    for k in range(case["K"]):
        if share:
            b = pkg.DeviceSharedReplayBuffer(U.args_of(case), case["A"], case["obs"], share, case["act"])
        else:
            b = pkg.DeviceReplayBuffer(U.args_of(case), case["A"], case["obs"], case["act"])
        U.feed(b, U.stream(case, k, share=share), lambda name, v, b=b: b.set_slot(name, 0, v))
        out.append(b)
    return out


def close(bufs):
    torch.cuda.synchronize()
    for b in bufs:
        b.close()


def host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def advantages_held(got, want):
    got, want = host(got), host(want)
    d = np.abs(got - want)
    print(f"advantages: max |d| {d.max():.3e}, max |x| {np.abs(want).max():.3e}")
    assert got.shape == want.shape and (d <= 2e-6 + 2e-6 * np.abs(want)).all()


def same_batches(got, want, names, what, loose_advantages=False):
    got, want = list(got), list(want)
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) == len(names), (what, i)
        for name, a, b in zip(names, g, w):
            a, b = host(a), host(b)
            assert a.dtype == np.float32 and a.shape == b.shape, (what, i, name, a.shape, b.shape)
            if name == "advantages" and loose_advantages:
                advantages_held(a, b)
            else:
                assert np.array_equal(a, b), (what, i, name)


def golden_batches(d, name, case):
    return [tuple(d[f"{name}/batch{i}_{j}"] for j in range(len(U.NAMES))) for i in range(case["n_mb"])]


# ---- the golden's cases
@pytest.mark.parametrize("name", list(U.CASES))
def test_golden_cases(pkg, name):
    case, d = U.CASES[name], golden()
    bufs = device_buffers(pkg, case)
    perm, want = d[f"{name}/perm"], golden_batches(d, name, case)
    gen = pkg.DeviceReplayBuffer.recurrent_generator
    for k, b in enumerate(bufs):
        assert np.array_equal(b.array("returns"), d[f"{name}/returns{k}"]), k
    same_batches(gen(bufs, case["n_mb"], case["L"], chunk_order=perm), want, U.NAMES, "generator, host arrays", True)
    same_batches(gen(bufs, case["n_mb"], case["L"], chunk_order=perm, on_device=True), want, U.NAMES, "generator, device tensors", True)
    torch.manual_seed(case["seed"])      # the permutation is the CPU generator's, as the reference's
    same_batches(gen(tuple(bufs), case["n_mb"], case["L"]), want, U.NAMES, "generator, drawn permutation", True)
    ep = pkg.DeviceReplayBuffer.epoch_of(bufs, case["n_mb"], case["L"], chunk_order=perm)
    torch.cuda.synchronize()
    assert isinstance(ep, pkg.DeviceEpoch) and len(ep) == case["n_mb"] and ep.names == U.NAMES
    mb = len(perm) // case["n_mb"]
    assert np.array_equal(host(ep.order), perm[:case["n_mb"] * mb].astype(np.int32))
    same_batches(ep, want, U.NAMES, "epoch_of", True)
    # each buffer's advantages are its own, and the restatement fed with them comes back bit for bit on every path
    adv = [b.array("advantages") for b in bufs]
    for k, a in enumerate(adv):
        advantages_held(a, d[f"{name}/advantages{k}"])
    exact = list(U.minibatches(U.oracle_buffers(case), perm, case["n_mb"], case["L"], advantages=adv))
    same_batches(ep, exact, U.NAMES, "epoch_of, the device's advantages")
    same_batches(gen(bufs, case["n_mb"], case["L"], chunk_order=perm), exact, U.NAMES, "generator, the device's advantages")
    ep2 = pkg.DeviceReplayBuffer.epoch_of(bufs, case["n_mb"], case["L"], chunk_order=torch.as_tensor(perm, device="cuda"))
    torch.cuda.synchronize()
    same_batches(ep2, exact, U.NAMES, "epoch_of, a device order")
    close(bufs)


def raw_gather(bufs, order, n_mb, mb, L):
    """ac_buffers_epoch_layout + ac_buffers_gather_epoch themselves: name -> [n_mb, rows, dim] arrays. (The Python entry points count
    n_rollout_threads * buffer_size * K // L chunks as the reference does; with agents the stack holds more, and the C calls reach them.)"""
    b = bufs[0]
    lib = b.lib
    handles = (C.c_void_p * len(bufs))(*[x._h for x in bufs])
    off, total = (C.c_int64 * 11)(), C.c_int64()
    assert lib.ac_buffers_epoch_layout(handles, len(bufs), n_mb, mb, L, off, C.byref(total)) == 0, lib.last_error()
    flat = torch.full((total.value,), float("nan"), device="cuda")
    d_order = torch.as_tensor(np.asarray(order, np.int32), device="cuda")
    torch.cuda.synchronize()
    for x in bufs:
        x.queue_advantages()
    assert lib.ac_buffers_gather_epoch(handles, len(bufs), None, d_order.data_ptr(), n_mb, mb, L, flat.data_ptr()) == 0, lib.last_error()
    torch.cuda.synchronize()
    flat = flat.cpu().numpy()
    names = U.SHARED_NAMES if b._shared else U.NAMES
    capi = importlib.import_module("aircombat-selfplay_amd.capi")
    out, covered = [], np.zeros(total.value, bool)
    for i in range(n_mb):
        item = []
        for name in names:
            dim = 1 if name == "advantages" else int(np.prod(b._shapes[name][3:]))
            rows = mb if name.startswith("rnn_states") else L * mb
            at = off[capi.AC_EPOCH_FIELDS.index(name)] + i * rows * dim
            item.append(flat[at:at + rows * dim].reshape(rows, dim))
            covered[at:at + rows * dim] = True
        out.append(tuple(item))
    assert not np.isnan(flat[covered]).any() and np.isnan(flat[~covered]).all()     # every field written, the padding never
    return out


def flat2(batches):
    return [tuple(a.reshape(a.shape[0], -1) for a in b) for b in batches]


@pytest.mark.parametrize("which", ["b-whole-stack", "K8", "tiles"])
def test_stack_shapes_against_the_restatement(pkg, which):
    case = {"b-whole-stack": U.CASES["b"], "K8": K8, "tiles": TILES}[which]
    bufs = device_buffers(pkg, case)
    K, T, N, L = case["K"], case["T"], case["E"] * case["A"], case["L"]
    n_chunks = K * T * N // L                                    # every chunk of the stack, the agents' rows included
    n_mb = case["n_mb"]
    mb = n_chunks // n_mb
    order = np.random.default_rng(case["seed"]).permutation(n_chunks)
    got = raw_gather(bufs, order, n_mb, mb, L)
    adv = [b.array("advantages") for b in bufs]
    ora = U.oracle_buffers(case)
    for a, o in zip(adv, ora):
        advantages_held(a, o.advantages)
    want = flat2(U.minibatches(ora, order, n_mb, L, advantages=adv, data_chunks=n_chunks))
    same_batches(got, want, U.NAMES, which)
    if which == "tiles":
        assert n_mb * mb * L == 160 and n_mb * mb == 80          # past one 64-row tile and no multiple of it, states included
    if which != "b-whole-stack":                                  # one agent: the Python entry points reach the same chunks
        data_chunks = case["E"] * (T * K) // L
        assert data_chunks == n_chunks
        want = list(U.minibatches(ora, order, n_mb, L, advantages=adv))
        ep = pkg.DeviceReplayBuffer.epoch_of(bufs, n_mb, L, chunk_order=order)
        torch.cuda.synchronize()
        same_batches(ep, want, U.NAMES, which + " epoch_of")
        same_batches(pkg.DeviceReplayBuffer.recurrent_generator(bufs, n_mb, L, chunk_order=order), want, U.NAMES, which + " generator")
    close(bufs)


def test_one_buffer_equals_epoch(pkg):
    case = dict(U.CASES["b"], K=1)
    (b,) = device_buffers(pkg, case)
    n_mb, L = case["n_mb"], case["L"]
    order = np.random.default_rng(1).permutation(case["E"] * case["T"] // L)
    single = b.epoch(n_mb, L, chunk_order=order)
    listed = pkg.DeviceReplayBuffer.epoch_of([b], n_mb, L, chunk_order=order)
    alone = pkg.DeviceReplayBuffer.epoch_of(b, n_mb, L, chunk_order=order)
    torch.cuda.synchronize()
    for ep in (listed, alone):
        assert ep.names == single.names and ep.flat.shape == single.flat.shape and np.array_equal(host(ep.order), host(single.order))
        same_batches(ep, single, U.NAMES, "epoch_of([b]) against b.epoch()")
    same_batches(pkg.DeviceReplayBuffer.recurrent_generator([b], n_mb, L, chunk_order=order, on_device=True), single, U.NAMES, "generator of [b]")
    close([b])


def test_shared_buffers(pkg):
    """The PPO list rule applied to the shared buffer's fields: 11 entries, share_obs and active_masks stacked like obs and masks."""
    case, share = SHARED, 16
    bufs = device_buffers(pkg, case, share=share)
    n_mb, L = case["n_mb"], case["L"]
    data_chunks = case["E"] * (case["T"] * case["K"]) // L
    order = np.random.default_rng(2).permutation(data_chunks)
    adv = [b.advantages for b in bufs]                           # (the property computes them; the calls below compute them again)
    ora = U.oracle_buffers(case, share=share)
    for a, o in zip(adv, ora):
        advantages_held(a, o.advantages)
    want = list(U.minibatches(ora, order, n_mb, L, advantages=adv))
    assert len(want[0]) == 11
    ep = pkg.DeviceReplayBuffer.epoch_of(bufs, n_mb, L, chunk_order=order)
    torch.cuda.synchronize()
    assert ep.names == U.SHARED_NAMES
    same_batches(ep, want, U.SHARED_NAMES, "shared epoch_of")
    same_batches(pkg.DeviceReplayBuffer.recurrent_generator(bufs, n_mb, L, chunk_order=order), want, U.SHARED_NAMES, "shared generator")
    same_batches(pkg.DeviceReplayBuffer.recurrent_generator(bufs, n_mb, L, chunk_order=order, on_device=True), want, U.SHARED_NAMES,
                 "shared generator, device tensors")
    close(bufs)


def test_device_order_is_clamped_into_the_stack(pkg):
    """A device order is used unchecked: -1 yields the first chunk of the stack, an index past the end the last one (memory safety)."""
    case = U.CASES["a"]
    bufs = device_buffers(pkg, case)
    K, T, N, L = case["K"], case["T"], case["E"] * case["A"], case["L"]
    n_chunks = K * T * N // L                                    # 22: the last chunk is rows 84 .. 87, in buffer 2
    order = np.arange(n_chunks)
    bad = order.copy()
    bad[3], bad[5], bad[8], bad[13] = -1, n_chunks, 2 ** 31 - 1, -2 ** 31
    fixed = order.copy()
    fixed[3], fixed[5], fixed[8], fixed[13] = 0, n_chunks - 1, n_chunks - 1, 0
    got = pkg.DeviceReplayBuffer.epoch_of(bufs, 1, L, chunk_order=torch.as_tensor(bad, device="cuda"))
    want = pkg.DeviceReplayBuffer.epoch_of(bufs, 1, L, chunk_order=torch.as_tensor(fixed, device="cuda"))
    torch.cuda.synchronize()
    same_batches(got, want, U.NAMES, "clamped order")
    exact = list(U.minibatches(U.oracle_buffers(case), fixed, 1, L, advantages=[b.array("advantages") for b in bufs]))
    same_batches(got, exact, U.NAMES, "clamped order against the restatement")
    assert U.source(n_chunks - 1, 0, L, T, N, K)[0] == K - 1
    with pytest.raises(RuntimeError, match="chunk index outside"):      # a host order is checked, as the single form checks it
        pkg.DeviceReplayBuffer.epoch_of(bufs, 1, L, chunk_order=bad)
    with pytest.raises(RuntimeError, match="chunk index outside the stack"):
        next(pkg.DeviceReplayBuffer.recurrent_generator(bufs, 1, L, chunk_order=bad))
    close(bufs)


# ---- refusals
def test_refusals_with_handles(pkg):
    case = U.CASES["a"]
    bufs = device_buffers(pkg, case)
    lib = bufs[0].lib
    capi = importlib.import_module("aircombat-selfplay_amd.capi")
    K, L, n_mb, mb = case["K"], case["L"], 2, 11
    arr = lambda bs: (C.c_void_p * len(bs))(*[None if b is None else b._h for b in bs])
    off, total = (C.c_int64 * 11)(), C.c_int64()
    order = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.zeros(1 << 14, device="cuda")
    chunks = np.zeros(4, np.int32)
    batch = capi.AcBufferBatch()
    torch.cuda.synchronize()
    # the layout is the single form's over K * T rows
    assert lib.ac_buffers_epoch_layout(arr(bufs), K, n_mb, mb, L, off, C.byref(total)) == 0
    cfg = capi.AcBufferConfig(case["T"] * K, case["E"], case["A"], case["obs"], 0, case["act"], 1, 1, case["hidden"], 1, 1, U.GAMMA, U.LAMBDA)
    off1, total1 = (C.c_int64 * 11)(), C.c_int64()
    assert lib.ac_buffer_epoch_layout_for(C.byref(cfg), n_mb, mb, L, off1, C.byref(total1)) == 0
    assert list(off) == list(off1) and total.value == total1.value and off[1] == -1 and off[4] == -1

    def other(**over):
        c = dict(case, **over)
        share = c.pop("share", 0)
        a = U.args_of(c)
        if share:
            return pkg.DeviceSharedReplayBuffer(a, c["A"], c["obs"], share, c["act"])
        return pkg.DeviceReplayBuffer(a, c["A"], c["obs"], c["act"])

    odd = {"buffer_size": other(T=9), "n_envs": other(E=4), "n_agents": other(A=2), "obs_dim": other(obs=6), "act_dim": other(act=3),
           "the RNN state's width": other(hidden=4), "shared versus unshared": other(share=10)}
    lists = [([bufs[0], None, bufs[2]], 3, "null handle"), (bufs, 0, "K must be in 1 .. 8"), (bufs * 3, 9, "K must be in 1 .. 8"),
             ([bufs[0], bufs[1], bufs[0]], 3, "the same handle twice")] + [([bufs[0], b], 2, "differ in " + what) for what, b in odd.items()]
    for bs, k, what in lists:
        for call in (lambda: lib.ac_buffers_epoch_layout(arr(bs), k, n_mb, 2, L, off, C.byref(total)),
                     lambda: lib.ac_buffers_gather_epoch(arr(bs), k, None, order.data_ptr(), n_mb, 2, L, out.data_ptr()),
                     lambda: lib.ac_buffers_minibatch(arr(bs), k, chunks.ctypes.data, 4, L, C.byref(batch), 1)):
            assert call() == -1
            assert what in lib.last_error(), (what, lib.last_error())
    h = arr(bufs)
    for call, what in ((lambda: lib.ac_buffers_gather_epoch(h, K, None, None, n_mb, mb, L, out.data_ptr()), "null argument"),
                       (lambda: lib.ac_buffers_gather_epoch(h, K, None, order.data_ptr(), n_mb, mb, L, None), "null argument"),
                       (lambda: lib.ac_buffers_gather_epoch(h, K, None, order.data_ptr(), 0, mb, L, out.data_ptr()), "must be positive"),
                       (lambda: lib.ac_buffers_gather_epoch(h, K, None, order.data_ptr(), n_mb, mb, -1, out.data_ptr()), "must be positive"),
                       # 90 rows: 2 * 11 * 4 = 88 fit, 2 * 12 * 4 = 96 do not
                       (lambda: lib.ac_buffers_gather_epoch(h, K, None, order.data_ptr(), n_mb, 12, L, out.data_ptr()), "exceeds the stack"),
                       (lambda: lib.ac_buffers_epoch_layout(h, K, n_mb, 12, L, off, C.byref(total)), "exceeds the stack"),
                       (lambda: lib.ac_buffers_epoch_layout(h, K, n_mb, mb, L, None, C.byref(total)), "null argument"),
                       (lambda: lib.ac_buffers_minibatch(h, K, None, 4, L, C.byref(batch), 1), "null argument"),
                       (lambda: lib.ac_buffers_minibatch(h, K, chunks.ctypes.data, 4, L, None, 1), "null argument"),
                       (lambda: lib.ac_buffers_minibatch(h, K, chunks.ctypes.data, 0, L, C.byref(batch), 1), "must be positive"),
                       (lambda: lib.ac_buffers_minibatch(h, K, np.array([0, 22, 1, 2], np.int32).ctypes.data, 4, L, C.byref(batch), 1),
                        "chunk index outside the stack")):
        assert call() == -1
        assert what in lib.last_error(), (what, lib.last_error())
    if torch.cuda.device_count() > 1:
        far = torch.cuda.Stream(device=1)
        assert lib.ac_buffers_gather_epoch(h, K, far.cuda_stream, order.data_ptr(), n_mb, mb, L, out.data_ptr()) == -1
        assert "another device" in lib.last_error()
        elsewhere = pkg.DeviceReplayBuffer(U.args_of(case), case["A"], case["obs"], case["act"], device_id=1)
        assert lib.ac_buffers_epoch_layout(arr([bufs[0], elsewhere]), 2, n_mb, 2, L, off, C.byref(total)) == -1
        assert "different devices" in lib.last_error()
        elsewhere.close()
    # the Python entry points raise with the library's message, and nothing was queued or broken: a valid call still works
    with pytest.raises(RuntimeError, match="the same handle twice"):
        pkg.DeviceReplayBuffer.epoch_of([bufs[0], bufs[0]], 2, L)
    with pytest.raises(RuntimeError, match="differ in buffer_size"):
        next(pkg.DeviceReplayBuffer.recurrent_generator([bufs[0], odd["buffer_size"]], 2, L))
    with pytest.raises(RuntimeError, match="K must be in 1 .. 8"):
        pkg.DeviceReplayBuffer.epoch_of(bufs * 3, 2, L)
    d, perm = golden(), golden()["a/perm"]
    ep = pkg.DeviceReplayBuffer.epoch_of(bufs, case["n_mb"], L, chunk_order=perm)
    torch.cuda.synchronize()
    same_batches(ep, golden_batches(d, "a", case), U.NAMES, "after the refusals", True)
    close(bufs + list(odd.values()))


# ---- two rollouts, one learner, one update
class Side:
    """An env handle of 4 singlecombat envs with its own buffer and collector; the learner's DevicePolicy is given (shared or its own)."""
    E, T = 4, 8

    def __init__(self, pkg, seed, policy):
        cfg = pkg.default_config("singlecombat")
        self.env = env = pkg.HipVecEnv(cfg, self.E, device_id=0, seed=seed)
        self.policy = policy
        self.buffer = pkg.DeviceReplayBuffer(learner_args(self.T, self.E), env.num_agents, env.observation_space, env.action_space)
        self.buffer.set_slot("obs", 0, env.reset())
        self.ro = pkg.DeviceRollout(env, policy, self.buffer, num_learner_agents=env.num_agents)

    def close(self):
        self.ro.close(); self.buffer.close(); self.env.close()


def learner_args(T, E):
    return types.SimpleNamespace(hidden_size="128 128", act_hidden_size="128 128", recurrent_hidden_size=128, recurrent_hidden_layers=1,
                                 activation_id=1, use_feature_normalization=False, use_prior=False, use_recurrent_policy=True, buffer_size=T,
                                 n_rollout_threads=E, gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False)


def device_policy(pkg, env, base, seed=11):
    P = importlib.import_module("aircombat-selfplay_amd.policy")
    pol = P.DevicePolicy(env.observation_space, env.action_space, learner_args(Side.T, Side.E), seed=seed)
    pol.load_from_torch(base.actor, base.critic)
    return pol


def swapped(pol):
    G = importlib.import_module("aircombat-selfplay_amd.gru_train")
    M = importlib.import_module("aircombat-selfplay_amd.mlp_train")
    A = importlib.import_module("aircombat-selfplay_amd.act_train")
    assert G.use_device_gru(pol) == 2 and M.use_device_mlp(pol) == 4 and A.use_device_act(pol) == 1
    return pol


def reference_form(pol):
    return types.SimpleNamespace(actor=pol.actor, critic=pol.critic, optimizer=pol.optimizer,
                                 evaluate_actions=lambda obs, ra, rc, a, m: pol.evaluate_actions(obs, obs, ra, rc, a, m))


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def held(what, dev, eager, f64):
    """tests/test_gpu_ppo_update.py's bound: rel(device) <= max(4 rel(torch fp32 eager on the same GPU), 2^-20), both against float64."""
    assert np.isfinite(np.asarray(dev, np.float64)).all(), what
    e_dev, e_ref = rel(dev, f64), rel(eager, f64)
    print(f"{what}: device {e_dev:.2e}, torch fp32 {e_ref:.2e}")
    assert e_dev <= max(4 * e_ref, FLOOR), (what, e_dev, e_ref)


def eager_update(pol, sample):
    """The reference-form update with torch, as tests/test_gpu_ppo_update.py restates it: the six values of PU.RETURNED."""
    obs, actions, masks, old_logp, adv, returns, vpreds, rnn_a, rnn_c = sample
    values, logp, ent = pol.evaluate_actions(obs, obs, rnn_a, rnn_c, actions, masks)
    st = PU.loss_torch(dict(values=values, action_log_probs=logp, dist_entropy=ent, old_action_log_probs=old_logp, advantages=adv, returns=returns,
                            value_preds=vpreds, active_masks=None), use_active=False)
    pol.optimizer.zero_grad()
    st["loss"].backward()
    an = torch.nn.utils.clip_grad_norm_(pol.actor.parameters(), 2.0)
    cn = torch.nn.utils.clip_grad_norm_(pol.critic.parameters(), 2.0)
    pol.optimizer.step()
    return [st[k].detach() for k in PU.RETURNED[:4]] + [an, cn]


def test_two_rollouts_share_one_learner_and_train_on_both(pkg):
    cfg = pkg.default_config("singlecombat")
    probe = pkg.HipVecEnv(cfg, Side.E, device_id=0, seed=1)
    P = importlib.import_module("aircombat-selfplay_amd.policy")
    nvec, n_shoot, _ = P._action_heads(probe.action_space)
    obs_dim = probe.obs_dim
    assert n_shoot == 0
    base = AU.Policy(seed=12, critic_obs=obs_dim, obs=obs_dim, nvec=tuple(int(n) for n in nvec))
    learner = device_policy(pkg, probe, base)
    learner.counter = 40
    sides = [Side(pkg, 7, learner), Side(pkg, 8, learner)]
    torch.cuda.synchronize()
    for s in sides:                       # one learner, two env handles: each collect takes the next T counters of the one policy
        assert s.ro.collect() == Side.T
        s.ro.compute_returns()
    assert learner.counter == 40 + 2 * Side.T
    torch.cuda.synchronize()
    # the rule of sharing: the second rollout is what a learner of its own with the same weights, seed and counter 40 + T collects
    own = device_policy(pkg, probe, base)
    own.counter = 40 + Side.T
    twin = Side(pkg, 8, own)
    twin.ro.collect()
    twin.ro.compute_returns()
    torch.cuda.synchronize()
    for name in ("obs", "actions", "rewards", "masks", "action_log_probs", "value_preds", "returns", "rnn_states_actor", "rnn_states_critic"):
        assert np.array_equal(sides[1].buffer.array(name), twin.buffer.array(name)), name
    assert not np.array_equal(sides[0].buffer.array("actions"), sides[1].buffer.array("actions"))
    twin.close(); own.close()

    bufs = [s.buffer for s in sides]
    L, n_mb, K = 4, 2, 2
    data_chunks = Side.E * (Side.T * K) // L
    orders = [np.random.default_rng(e).permutation(data_chunks) for e in range(2)]
    runs = {}
    for kind, kw in (("default", {}), ("stream", dict(stream_ordered=True))):
        pol = swapped(copy.deepcopy(base))
        tr = pkg.DevicePPOTrainer(PU.trainer_args(data_chunk_length=L), torch.device("cuda", 0))
        assert tr.ppo_epoch == 2 and tr.num_mini_batch == n_mb
        info = tr.train(reference_form(pol), bufs, chunk_orders=orders, **kw)
        torch.cuda.synchronize()
        runs[kind] = (info, [p.detach().cpu().numpy() for p in list(pol.actor.parameters()) + list(pol.critic.parameters())])
    (want_info, want_p), (info, params) = runs["default"], runs["stream"]
    assert list(want_info) == ["value_loss", "policy_loss", "policy_entropy_loss", "actor_grad_norm", "critic_grad_norm", "ratio"]
    assert info == want_info, (info, want_info)                                      # float for float
    assert all(np.array_equal(a, b) for a, b in zip(params, want_p))
    before = [p.detach().cpu().numpy() for p in list(base.actor.parameters()) + list(base.critic.parameters())]
    assert any(not np.array_equal(a, b) for a, b in zip(want_p, before))
    # the torch restatement on the concatenated mini-batches: the numpy stack of the two buffers' arrays, cut by the same orders
    from oracle.rollout_buffer import OracleRolloutBuffer
    mirrors = []
    for b in bufs:
        m = OracleRolloutBuffer(Side.T, Side.E, b.num_agents, obs_dim, len(nvec), 1, 128, 0.99, 0.95, True, False)
        for name in ("obs", "actions", "rewards", "masks", "bad_masks", "action_log_probs", "value_preds", "returns", "rnn_states_actor",
                     "rnn_states_critic"):
            getattr(m, name)[...] = b.array(name)
        mirrors.append(m)
    adv = [b.array("advantages") for b in bufs]
    loops = {}
    for kind in ("torch", "f64"):
        pol, rows = copy.deepcopy(base), []
        if kind == "f64":
            pol.actor.double(); pol.critic.double()
        for e in range(2):
            for sample in U.minibatches(mirrors, orders[e], n_mb, L, advantages=adv):
                s = tuple(torch.as_tensor(x).cuda() for x in sample)
                s = tuple(t.double() for t in s) if kind == "f64" else s
                rows.append([float(x) for x in eager_update(pol, s)])
        assert len(rows) == 4
        loops[kind] = dict(zip(PU.RETURNED, np.asarray(rows, np.float64).sum(0) / 4))
    losses = ("policy_loss", "value_loss", "policy_entropy_loss")
    held("train on two buffers, losses", *[[d[k] for k in losses] for d in (want_info, loops["torch"], loops["f64"])])
    for k in ("ratio", "actor_grad_norm", "critic_grad_norm"):
        held(f"train on two buffers, {k}", want_info[k], loops["torch"][k], loops["f64"][k])
    for s in sides:
        s.close()
    learner.close(); probe.close()
