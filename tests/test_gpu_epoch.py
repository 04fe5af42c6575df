"""The stream-ordered hand-over on the MI355X (include/aircombat_epoch.h, csrc/epoch_gather.hpp; buffer.compute_returns(wait=False),
queue_advantages, epoch, DeviceRollout.compute_returns(wait=False), DevicePPOTrainer.train(stream_ordered=True)) against the blocking
calls it stands beside. The new path moves the same floats and runs the same arithmetic kernels, so every comparison is bit for bit
(np.array_equal); nothing here has a tolerance.

One remark on "the same arithmetic": the advantage statistics are fp64 block sums added with atomics, so with more than one block
(more than 256 entries) two runs may add them in another order; a difference of an fp64 ulp in a sum would have to flip the
rounding of the float32 mean or deviation to show. The tests compare such runs as equal all the same.

The shapes are the smallest at which the index arithmetic can go wrong (see SHAPES). No test feeds an out-of-range index to the
device: the kernel's clamp is tested on the host (tests/test_epoch_host.py)."""
import copy
import ctypes as C
import importlib
import types

import numpy as np
import pytest

import act_train_util as AU
import mlp_train_util as MU
import policy_util as PU
import ppo_update_util as U

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OBS, ACT, H = 21, 7, 128
# T, E, A, L, n_mb, share_obs_dim
SHAPES = {
    "straddle": (7, 3, 2, 4, 2, 42),      # T % L != 0: chunks straddle columns; 5 chunks -> mb = 2, one chunk dropped; odd dims
    "L1": (5, 2, 1, 1, 3, 42),            # L = 1, mb no divisor of the chunks
    "one-mb": (8, 4, 2, 8, 1, 42),        # one mini-batch, L = T
    "tiles": (64, 33, 2, 8, 5, 42),       # 1320 rows: crosses the kernel's 64-row tile, ragged last tile
    "tiles-odd-share": (64, 33, 2, 8, 5, 43),   # share_obs rows of 43 floats: the 16-byte path must not be taken
    "tiles-vec-share": (64, 33, 2, 8, 5, 44),   # share_obs rows of 44 floats: 11 float4 units per row, the 16-byte path across tiles
}
PER_STEP = ("obs", "share_obs", "actions", "rewards", "masks", "bad_masks", "active_masks", "action_log_probs", "value_preds", "returns",
            "rnn_states_actor", "rnn_states_critic")


def _args(T, E, gae=True, proper=False):
    return types.SimpleNamespace(buffer_size=T, n_rollout_threads=E, gamma=0.99, use_proper_time_limits=proper, use_gae=gae, gae_lambda=0.95,
                                 recurrent_hidden_size=H, recurrent_hidden_layers=1)


def make(pkg, shared, T, E, A, share=42, gae=True, proper=False):
    if shared:
        return pkg.DeviceSharedReplayBuffer(_args(T, E, gae, proper), A, OBS, share, ACT)
    return pkg.DeviceReplayBuffer(_args(T, E, gae, proper), A, OBS, ACT)


def contents(buf, seed, pattern=False):
    """name -> float32 array of the buffer's shape. ``pattern``: every element names its field, source row and column,
    code = field * 2^20 + (t * N + col) * 128 + k (< 2^24: exact in float32), so that a misplaced row names where it came from."""
    rng = np.random.default_rng(seed)
    out = {}
    for f, name in enumerate(n for n in PER_STEP if n in buf._shapes):
        shape = buf._shapes[name]
        if pattern:
            rows, k = int(np.prod(shape[:3])), int(np.prod(shape[3:]))
            out[name] = (f * 2 ** 20 + np.arange(rows)[:, None] * 128 + np.arange(k)[None, :]).astype(np.float32).reshape(shape)
        elif name.endswith("masks"):
            out[name] = (rng.random(shape) > 0.1).astype(np.float32)
        else:
            out[name] = rng.normal(size=shape).astype(np.float32)
    return out


def fill(buf, data):
    for name, a in data.items():
        buf.device_tensor(name).copy_(torch.from_numpy(a))
    torch.cuda.synchronize()   # the buffer's blocking calls run on its own stream


def mirror(buf, shared, data, share):
    """The numpy buffer of the existing buffer tests with the same contents."""
    from oracle.rollout_buffer import OracleRolloutBuffer
    T, E, A = buf.buffer_size, buf.n_rollout_threads, buf.num_agents
    ref = OracleRolloutBuffer(T, E, A, OBS, ACT, 1, H, 0.99, 0.95, buf.use_gae, buf.use_proper_time_limits, share_dim=share if shared else 0)
    for name, a in data.items():
        getattr(ref, name)[...] = a
    return ref


def same(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


# ---- 2. the gather
@pytest.mark.parametrize("shared", [False, True], ids=["ppo", "shared"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_epoch_equals_the_minibatches(pkg, shape, shared):
    T, E, A, L, n_mb, share = SHAPES[shape]
    buf = make(pkg, shared, T, E, A, share)
    data = contents(buf, seed=3, pattern=shape == "straddle")
    fill(buf, data)
    if shape != "straddle":   # (the pattern keeps its `returns`; the advantages are computed from them either way)
        buf.compute_returns(torch.from_numpy(np.random.default_rng(4).normal(size=E * A).astype(np.float32)).cuda(), on_device=True)
    data_chunks = E * T // L
    mb = data_chunks // n_mb
    order = np.random.default_rng(5).permutation(data_chunks)
    ep = buf.epoch(n_mb, L, chunk_order=order)
    torch.cuda.synchronize()
    names = buf._BATCH + ("rnn_states_actor", "rnn_states_critic")
    assert isinstance(ep, pkg.DeviceEpoch) and len(ep) == n_mb and ep.names == names and len(names) == (11 if shared else 9)
    assert ep.order.dtype == torch.int32 and ep.order.is_cuda and same(ep.order, order[:n_mb * mb].astype(np.int32))
    assert ep.flat.dtype == torch.float32 and ep.flat.dim() == 1
    lo, hi = ep.flat.data_ptr(), ep.flat.data_ptr() + 4 * ep.flat.numel()
    ref = mirror(buf, shared, {k: buf.array(k) for k in data}, share)
    want_ref = list(ref.minibatches(order, n_mb, L, advantages=buf.array("advantages")))
    items = list(ep)
    assert len(items) == n_mb
    for i in range(n_mb):
        want = buf.minibatch(order[i * mb:(i + 1) * mb], L, on_device=True)
        assert len(ep[i]) == len(want) == len(want_ref[i]) == len(names) and items[i] is ep[i]
        for name, got, w, r in zip(names, ep[i], want, want_ref[i]):
            assert got.dtype == w.dtype and got.shape == w.shape and got.device == w.device and got.is_contiguous(), (i, name)
            assert lo <= got.data_ptr() and got.data_ptr() + 4 * got.numel() <= hi, (i, name)     # a view into the flat tensor
            assert same(got, w), (shape, i, name, "against minibatch(on_device=True)")
            assert same(got, r.reshape(w.shape)), (shape, i, name, "against the numpy buffer's minibatches")
    if shape == "straddle":   # the pattern, read back: row l * mb + j of mini-batch i names step l of chunk order[i * mb + j]
        N = E * A
        obs = ep[1][0].cpu().numpy()
        for l in range(L):
            for j in range(mb):
                row = int(order[mb + j]) * L + l
                assert obs[l * mb + j, 0] == 0 * 2 ** 20 + ((row % T) * N + row // T) * 128, (l, j)
    # an integer tensor on the device is used as it is
    ep2 = buf.epoch(n_mb, L, chunk_order=torch.as_tensor(order, device="cuda"))
    torch.cuda.synchronize()
    assert same(ep2.order, ep.order) and ep2.flat.shape == ep.flat.shape
    assert all(same(x, y) for i in range(n_mb) for x, y in zip(ep2[i], ep[i]))   # (the padding between fields is never written)
    buf.close()


def test_refusals_with_a_handle(pkg):
    T, E, A, L, n_mb, share = SHAPES["straddle"]
    buf = make(pkg, False, T, E, A)
    lib, h = buf.lib, buf._h
    order = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.zeros(1 << 16, device="cuda")
    torch.cuda.synchronize()
    off, total = (C.c_int64 * 11)(), C.c_int64()
    assert lib.ac_buffer_epoch_layout(h, n_mb, 2, L, off, C.byref(total)) == 0
    assert off[1] == -1 and off[4] == -1 and total.value > 0 and all(o % 4 == 0 for o in off if o >= 0)
    for call, what in ((lambda: lib.ac_buffer_gather_epoch(h, None, None, n_mb, 2, L, out.data_ptr()), "null argument"),
                       (lambda: lib.ac_buffer_gather_epoch(h, None, order.data_ptr(), n_mb, 2, L, None), "null argument"),
                       (lambda: lib.ac_buffer_gather_epoch(h, None, order.data_ptr(), 0, 2, L, out.data_ptr()), "must be positive"),
                       (lambda: lib.ac_buffer_gather_epoch(h, None, order.data_ptr(), n_mb, 0, L, out.data_ptr()), "must be positive"),
                       (lambda: lib.ac_buffer_gather_epoch(h, None, order.data_ptr(), n_mb, 2, -3, out.data_ptr()), "must be positive"),
                       # T * N = 42 rows: 2 * 6 * 4 = 48 do not fit
                       (lambda: lib.ac_buffer_gather_epoch(h, None, order.data_ptr(), n_mb, 6, L, out.data_ptr()), "exceeds the buffer"),
                       (lambda: lib.ac_buffer_epoch_layout(h, n_mb, 6, L, off, C.byref(total)), "exceeds the buffer"),
                       (lambda: lib.ac_buffer_compute_returns_on(h, None, None), "null argument")):
        assert call() == -1
        assert what in lib.last_error(), (what, lib.last_error())
    if torch.cuda.device_count() > 1:   # a stream of another device than the buffer's
        other = torch.cuda.Stream(device=1)
        for call in (lambda: lib.ac_buffer_gather_epoch(h, other.cuda_stream, order.data_ptr(), n_mb, 2, L, out.data_ptr()),
                     lambda: lib.ac_buffer_advantages_on(h, other.cuda_stream),
                     lambda: lib.ac_buffer_compute_returns_on(h, other.cuda_stream, out.data_ptr())):
            assert call() == -1 and "another device" in lib.last_error()
    with pytest.raises(RuntimeError, match="chunk index outside"):     # a host order is checked on the host, as minibatch checks it
        buf.epoch(n_mb, L, chunk_order=[0, 1, 2, 11])                   # chunk 11 would end at row 48 > 42
    with pytest.raises(RuntimeError, match="chunk index outside"):
        buf.epoch(n_mb, L, chunk_order=[0, -1, 2, 3])
    with pytest.raises(ValueError):
        buf.epoch(n_mb, L, chunk_order=[0, 1, 2])                       # 4 are needed
    with pytest.raises(ValueError):
        buf.epoch(n_mb, L, chunk_order=torch.zeros(4, device="cuda"))   # a float tensor is no index array
    with pytest.raises(ValueError):
        buf.compute_returns(np.zeros(E * A, np.float32), wait=False)    # a host array could be reused before it is read
    torch.cuda.synchronize()
    buf.close()


# ---- 3. returns and advantages
@pytest.mark.parametrize("gae", [False, True], ids=["mc", "gae"])
@pytest.mark.parametrize("proper", [False, True], ids=["plain", "proper"])
@pytest.mark.parametrize("shared", [False, True], ids=["ppo", "shared"])
@pytest.mark.parametrize("shape", ["straddle", "tiles"])
def test_queued_returns_and_advantages_equal_the_blocking_ones(pkg, shape, shared, proper, gae):
    T, E, A, L, n_mb, share = SHAPES[shape]
    a, b = (make(pkg, shared, T, E, A, share, gae=gae, proper=proper) for _ in range(2))
    data = contents(a, seed=11)
    fill(a, data); fill(b, data)
    nv = torch.from_numpy(np.random.default_rng(12).normal(size=E * A).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    a.compute_returns(nv, on_device=True)
    adv_a = a.advantages
    b.compute_returns(nv, on_device=True, wait=False)
    b.queue_advantages()
    torch.cuda.synchronize()
    assert same(a.array("returns"), b.array("returns"))
    assert same(a.array("value_preds")[-1], b.array("value_preds")[-1])
    assert same(a.array("returns")[-1] if not gae else a.array("value_preds")[-1], nv.cpu().numpy().reshape(E, A, 1))
    assert same(adv_a, b.array("advantages")) and np.isfinite(adv_a).all() and np.abs(adv_a).max() > 0
    a.close(); b.close()


# ---- 4. ordering without waits
@pytest.fixture(scope="module")
def blocker_cycles():
    """torch.cuda._sleep cycles for about 0.2 s, measured once with events."""
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    probe = 10_000_000
    t0.record(); torch.cuda._sleep(probe); t1.record()
    torch.cuda.synchronize()
    return int(probe * 200.0 / max(t0.elapsed_time(t1), 1e-3))


def test_ordering_without_waits(pkg, blocker_cycles):
    T, E, A, L, n_mb, share = SHAPES["straddle"]
    buf, twin = make(pkg, False, T, E, A), make(pkg, False, T, E, A)
    data = contents(buf, seed=21)
    fill(buf, data)
    new_obs = np.random.default_rng(22).normal(size=data["obs"].shape).astype(np.float32)
    fill(twin, {**data, "obs": new_obs})
    d_new = torch.from_numpy(new_obs).cuda()
    nv = torch.from_numpy(np.random.default_rng(23).normal(size=E * A).astype(np.float32)).cuda()
    order = np.random.default_rng(24).permutation(E * T // L)
    mb = len(order) // n_mb
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        buf.epoch(n_mb, L, chunk_order=order)      # once before, so that the allocators' first use is not what is timed
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    with torch.cuda.stream(side):
        torch.cuda._sleep(blocker_cycles)
        buf.device_tensor("obs").copy_(d_new, non_blocking=True)
        buf.compute_returns(nv, on_device=True, wait=False)
        ep = buf.epoch(n_mb, L, chunk_order=order)
        done.record(side)
    assert done.query() is False                   # the calls returned while the blocker was still running: nothing waited
    side.synchronize()
    assert done.query() is True
    twin.compute_returns(nv, on_device=True)
    twin.advantages
    assert same(buf.array("returns"), twin.array("returns"))
    for i in range(n_mb):
        want = twin.minibatch(order[i * mb:(i + 1) * mb], L, on_device=True)
        for name, got, w in zip(ep.names, ep[i], want):
            assert same(got, w), (i, name)         # the overwritten observations, the returns queued behind them
    from oracle.rollout_buffer import OracleRolloutBuffer
    rows = (order[:mb][None, :] * L + np.arange(L)[:, None]).reshape(-1)
    assert same(ep[0][0], OracleRolloutBuffer.sequence_rows(new_obs[:-1])[rows])
    assert not same(ep[0][0], OracleRolloutBuffer.sequence_rows(data["obs"][:-1])[rows])      # not what was there before the blocker
    buf.after_update()                            # a blocking call on the buffer's own stream, ordered after the gather
    assert same(buf.array("obs")[0], new_obs[-1])
    buf.close(); twin.close()


# ---- 5 / 6. the trainer
def _filled_buffer(pkg, shared, T=32, E=32, L=8, seed=5):
    """The buffer of test_gpu_ppo_update.py's train test: T = 32 steps of E = 32 envs, chunks of L = 8, the restated policy's dims."""
    obs, nvec = MU.OBS, MU.NVEC
    args = _args(T, E)
    buf = pkg.DeviceSharedReplayBuffer(args, 2, obs, 2 * obs, len(nvec)) if shared else pkg.DeviceReplayBuffer(args, 1, obs, len(nvec))
    gen = torch.Generator(device="cuda").manual_seed(seed)
    for name in ("obs", "rewards", "action_log_probs", "value_preds", "rnn_states_actor", "rnn_states_critic") + (("share_obs",) if shared else ()):
        buf.device_tensor(name).normal_(generator=gen)
    buf.device_tensor("action_log_probs").mul_(0.1).sub_(2.0)
    a = buf.device_tensor("actions")
    for i, n in enumerate(nvec):
        a[..., i] = torch.randint(0, n, a[..., i].shape, device="cuda", generator=gen).float()
    buf.device_tensor("masks").copy_((torch.rand(buf.device_tensor("masks").shape, device="cuda", generator=gen) > 0.05).float())
    if shared:
        buf.device_tensor("active_masks").copy_((torch.rand(buf.device_tensor("active_masks").shape, device="cuda", generator=gen) > 0.1).float())
    nv = torch.randn(E * buf.num_agents, device="cuda", generator=gen)
    torch.cuda.synchronize()
    buf.compute_returns(nv, on_device=True)
    torch.cuda.synchronize()
    return buf, T * E // L, L


def _swapped(pol):
    G = importlib.import_module("aircombat-selfplay_amd.gru_train")
    M = importlib.import_module("aircombat-selfplay_amd.mlp_train")
    A = importlib.import_module("aircombat-selfplay_amd.act_train")
    assert G.use_device_gru(pol) == 2 and M.use_device_mlp(pol) == 4 and A.use_device_act(pol) == 1
    return pol


def _as_reference_policy(pol, shared):
    if shared:
        return pol
    return types.SimpleNamespace(actor=pol.actor, critic=pol.critic, optimizer=pol.optimizer,
                                 evaluate_actions=lambda obs, ra, rc, a, m: pol.evaluate_actions(obs, obs, ra, rc, a, m))


def _trainer(pkg, shared, **over):
    return pkg.DevicePPOTrainer(U.trainer_args(use_policy_active_masks=shared, **over), torch.device("cuda", 0))


def test_no_torch_side_synchronisation(pkg):
    buf, nchunks, L = _filled_buffer(pkg, False, seed=9)
    pol = _swapped(AU.Policy(seed=13))
    ref_pol, tr = _as_reference_policy(pol, False), _trainer(pkg, False)
    orders = []
    for run in range(2):
        torch.manual_seed(77)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            ep = buf.epoch(2, L, chunk_order=None)
            if run == 0:
                first, second = tr.ppo_update(ref_pol, ep[0]), tr.ppo_update(ref_pol, ep[1])
                with pytest.raises(RuntimeError):   # a torch call that does synchronise raises under the same mode: the check is live
                    second[0].item()
        finally:
            torch.cuda.set_sync_debug_mode(0)
        torch.cuda.synchronize()
        orders.append(ep.order.cpu().numpy())
    assert all(torch.isfinite(x) for x in first + second)
    o = orders[0]
    assert o.dtype == np.int32 and len(o) == 2 * (nchunks // 2) and len(set(o.tolist())) == len(o) and o.min() >= 0 and o.max() < nchunks
    assert not np.array_equal(o, np.sort(o))          # a permutation's prefix, and a drawn one
    assert np.array_equal(orders[0], orders[1])       # torch.manual_seed seeds the device generator it is drawn from
    buf.close()


@pytest.mark.parametrize("shared", [False, True], ids=["own-obs", "share-obs"])
def test_train_stream_ordered_equals_the_default(pkg, shared):
    buf, nchunks, L = _filled_buffer(pkg, shared, seed=7 + shared)
    orders = [np.random.default_rng(e).permutation(nchunks) for e in range(2)]
    base = AU.Policy(seed=12, critic_obs=2 * MU.OBS if shared else MU.OBS)
    runs = {}
    for kind, kw in (("default", {}), ("stream", dict(stream_ordered=True)), ("args", {})):
        pol = _swapped(copy.deepcopy(base))
        tr = _trainer(pkg, shared, data_chunk_length=L, **({"use_stream_ordered_minibatches": True} if kind == "args" else {}))
        assert tr.ppo_epoch == 2 and tr.num_mini_batch == 2
        info = tr.train(_as_reference_policy(pol, shared), buf, chunk_orders=orders, **kw)
        torch.cuda.synchronize()
        runs[kind] = (info, [p.detach().cpu().numpy() for p in list(pol.actor.parameters()) + list(pol.critic.parameters())])
    want_info, want_p = runs["default"]
    assert list(want_info) == ["value_loss", "policy_loss", "policy_entropy_loss", "actor_grad_norm", "critic_grad_norm", "ratio"]
    for kind in ("stream", "args"):
        info, params = runs[kind]
        assert info == want_info, (kind, info, want_info)                       # float for float
        assert all(np.array_equal(a, b) for a, b in zip(params, want_p)), kind
    assert any(not np.array_equal(a, b.detach().cpu().numpy()) for a, b in zip(want_p, list(base.actor.parameters()) + list(base.critic.parameters())))
    from oracle.rollout_buffer import OracleRolloutBuffer
    host_buffer = OracleRolloutBuffer(8, 4, 1, MU.OBS, len(MU.NVEC), 1, H, 0.99, 0.95, True, False)
    with pytest.raises(ValueError, match="stream_ordered"):
        _trainer(pkg, shared, data_chunk_length=L).train(_as_reference_policy(_swapped(copy.deepcopy(base)), shared), host_buffer, stream_ordered=True)
    buf.close()


# ---- 7. the rollout
class Side:
    """env, learner and buffer of a 1v1 rollout; two Sides are built alike (tests/test_gpu_rollout_collect.py's handles)."""
    E, T = 5, 8

    def __init__(self, pkg):
        P = importlib.import_module("aircombat-selfplay_amd.policy")
        cfg = pkg.default_config("singlecombat")
        cfg.max_steps = 5
        self.env = env = pkg.HipVecEnv(cfg, self.E, device_id=0, seed=7)
        nvec, n_shoot, _ = P._action_heads(env.action_space)
        a = types.SimpleNamespace(hidden_size="128 128", act_hidden_size="128 128", recurrent_hidden_size=128, recurrent_hidden_layers=1,
                                  activation_id=1, use_feature_normalization=True, use_prior=n_shoot > 0, use_recurrent_policy=True,
                                  buffer_size=self.T, n_rollout_threads=self.E, gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False)
        self.policy = P.DevicePolicy(env.observation_space, env.action_space, a, seed=11)
        self.policy.load_state_dict(*PU.seeded_state_dicts(env.obs_dim, nvec, True, seed=1201))
        self.policy.counter = 40
        self.buffer = pkg.DeviceReplayBuffer(a, env.num_agents, env.observation_space, env.action_space)
        self.buffer.set_slot("obs", 0, env.reset())
        self.ro = pkg.DeviceRollout(env, self.policy, self.buffer, num_learner_agents=env.num_agents)

    def close(self):
        self.ro.close(); self.buffer.close(); self.env.close()


def test_rollout_compute_returns_without_a_wait(pkg):
    a, b = Side(pkg), Side(pkg)
    torch.cuda.synchronize()
    a.ro.collect()
    nv_a = a.ro.compute_returns()
    b.ro.collect()
    nv_b = b.ro.compute_returns(wait=False)
    torch.cuda.synchronize()
    a.env.sync(); b.env.sync()
    assert same(nv_a, nv_b)
    for name in ("obs", "rewards", "value_preds", "returns"):
        assert same(a.buffer.array(name), b.buffer.array(name)), name
    assert np.abs(a.buffer.array("returns")).max() > 0
    a.close(); b.close()
