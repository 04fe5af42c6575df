"""The opponent pool (DevicePolicyPool, csrc/policy_pool.hpp) on the MI355X: every member's rows bit-identical to a DevicePolicy /
actor-only DeviceMAPPOPolicy holding that member in the same call, the golden 1v1 actor as a member, untouched unassigned rows, the load
paths, sizes, stream order, and a device rollout with the pool on the opponents' agent range."""
import importlib
import types

import numpy as np
import pytest

import policy_util as U

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = {"fast": {"logp": 2e-5, "h": 4.2e-6}, "fp32": {"logp": 1e-5, "h": 2.1e-6}}   # test_gpu_policy.py's
MARGIN = 1e-4


@pytest.fixture(scope="module")
def P(pkg):
    return importlib.import_module("aircombat-selfplay_amd.policy")


def args(fn, prior):
    return types.SimpleNamespace(hidden_size="128 128", act_hidden_size="128 128", recurrent_hidden_size=128, recurrent_hidden_layers=1,
                                 activation_id=1, use_feature_normalization=fn, use_prior=prior, use_recurrent_policy=True)


def member_sd(obs_dim, nvec, n_shoot, fn, seed):
    """policy_util's seeded actor (one hash stream per tensor), plus munition heads when the action space has them."""
    return U.add_munition_heads(U.seeded_state_dicts(obs_dim, nvec, fn, seed=seed)[0], len(nvec), n_shoot, seed)


def heads(act_space):
    P = importlib.import_module("aircombat-selfplay_amd.policy")
    nvec, n_shoot, _ = P._action_heads(act_space)
    return nvec, n_shoot


def make_env(pkg, form, E, seed=3):
    if form == "ppo":   # 1v1: the learner on agent 0, the opponents on agent 1
        return pkg.HipVecEnv(pkg.default_config("singlecombat"), E, device_id=0, seed=seed), slice(1, 2)
    return pkg.HipShareVecEnv(pkg.default_config("scenario2_nvn"), E, device_id=0, seed=seed), slice(2, 4)   # 2v2


def single(P, env, form, sd, precision, seed):
    """The one-member reference: DevicePolicy (ppo) or actor-only DeviceMAPPOPolicy (mappo) holding sd."""
    nvec, n_shoot = heads(env.action_space)
    a = args(form == "ppo", n_shoot > 0)
    if form == "ppo":
        p = P.DevicePolicy(env.observation_space, env.action_space, a, precision=precision, seed=seed, critic=False)
    else:
        cent = importlib.import_module("aircombat-selfplay_amd.vec_env")._Box(-10, 10, (env.num_agents * env.obs_dim,))
        p = P.DeviceMAPPOPolicy(env.observation_space, cent, env.action_space, a, precision=precision, seed=seed, critic=False)
    p.load_state_dict(sd)
    return p


def pool_for(P, env, form, precision, capacity, seed):
    nvec, n_shoot = heads(env.action_space)
    return P.DevicePolicyPool(env.observation_space, env.action_space, args(form == "ppo", n_shoot > 0), capacity, form=form,
                              precision=precision, seed=seed)


def random_inputs(env, agents, rng):
    """Random observations written into the env's device obs buffer (every row differs), random GRU states and masks."""
    _, obs_d, _, _, _ = env.device_tensors()
    obs_d.copy_(torch.as_tensor(rng.normal(0, 0.6, tuple(obs_d.shape)).astype(np.float32)).cuda())
    a0, a1, _ = agents.indices(env.num_agents)
    n = env.num_envs * (a1 - a0)
    h = torch.as_tensor(rng.normal(0, 0.5, (n, 1, 128)).astype(np.float32)).cuda()
    m = torch.as_tensor((rng.random((n, 1)) > 0.2).astype(np.float32)).cuda()
    return h, m


@pytest.mark.parametrize("precision", ["fast", "fp32"])
@pytest.mark.parametrize("form", ["ppo", "mappo"])
def test_members_match_single_policies(P, pkg, form, precision):
    E = 200
    env, agents = make_env(pkg, form, E)
    env.reset()
    nvec, n_shoot = heads(env.action_space)
    a0, a1, _ = agents.indices(env.num_agents)
    na, nh = a1 - a0, len(nvec) + n_shoot
    rng = np.random.default_rng(11)
    h, m = random_inputs(env, agents, rng)
    act_d = env.device_tensors()[0]
    sds = [member_sd(env.obs_dim, nvec, n_shoot, form == "ppo", 500 + k) for k in range(8)]
    pool = pool_for(P, env, form, precision, 8, seed=77)
    for k, sd in enumerate(sds):
        pool.load_state_dict(k, sd)
    refs = [single(P, env, form, sd, precision, 77) for sd in sds]
    for K in (1, 3, 8):
        members = rng.integers(0, K, E).astype(np.int32)   # non-contiguous
        pool.assign(members)
        for det in (True, False):
            counter = 10 + K
            outs = []
            for xcd in (False, True):
                pool.set_tile_order(xcd)
                ho, lp = pool.act_into_env(env, h, m, agents=agents, deterministic=det, counter=counter, rnn_states_out=torch.empty_like(h))
                outs.append((act_d[:, a0:a1, :nh].clone(), ho, lp))
            torch.cuda.current_stream().synchronize()
            for x, y in zip(*outs):   # the tile order changes no bit
                assert torch.equal(x, y)
            act_pool, ho_pool, lp_pool = outs[0]
            for k in range(K):
                rows_e = torch.as_tensor(np.nonzero(members == k)[0]).cuda()
                rows = (rows_e[:, None] * na + torch.arange(na, device="cuda")[None, :]).reshape(-1)
                if rows.numel() == 0:
                    continue
                hr, lr = refs[k].act_into_env(env, h, m, agents=agents, deterministic=det, counter=counter, rnn_states_out=torch.empty_like(h))
                torch.cuda.current_stream().synchronize()
                ar = act_d[:, a0:a1, :nh]
                tag = f"K={K} det={det} member {k}"
                assert torch.equal(act_pool[rows_e], ar[rows_e]), tag
                assert torch.equal(ho_pool[rows], hr[rows]), tag
                assert torch.equal(lp_pool[rows], lr[rows]), tag
    for p in refs + [pool]:
        p.close()
    env.close()


def ambiguous(g):
    nvec, n_shoot = U.CASES["a"][1], U.CASES["a"][2]
    lg, cols, off = g["a_logits"], [], 0
    for n in nvec:
        s = np.sort(lg[:, off:off + n], -1)
        cols.append(s[:, -1] - s[:, -2] < MARGIN)
        off += n
    for k in range(n_shoot):
        cols.append(np.abs(g["a_shoot_p"][:, k] - 0.5) < MARGIN)
    return np.stack(cols, -1)


@pytest.mark.parametrize("precision", ["fast", "fp32"])
def test_golden_member(P, precision):
    g = U.golden()
    obs_s, act_s = U.spaces("a")
    asd, _ = U.state_dicts(g, "a")
    obs_dim, nvec, n_shoot = U.CASES["a"][:3]
    pool = P.DevicePolicyPool(obs_s, act_s, U.args("a"), 3, precision=precision)
    pool.load_state_dict(0, member_sd(obs_dim, nvec, n_shoot, False, 601))
    pool.load_state_dict(1, asd)
    pool.load_state_dict(2, member_sd(obs_dim, nvec, n_shoot, False, 602))
    n = len(g["a_obs"])
    members = np.where(np.arange(n) % 3 == 0, np.arange(n) % 2 * 2, 1).astype(np.int32)
    pool.assign(members)
    a, ha, lp = pool.act(g["a_obs"], g["a_rnn_states"], g["a_masks"], deterministic=True, return_log_probs=True)
    sel = members == 1
    amb = ambiguous(g)
    ok = (a[sel] == g["a_actions"][sel]) | amb[sel]
    assert ok.all(), f"{(~ok).sum()} actions differ outside tie margins"
    exact = (a[sel] == g["a_actions"][sel]).all(-1)
    assert np.abs(lp[sel] - g["a_log_probs"][sel])[exact].max() < TOL[precision]["logp"]
    assert np.abs(ha[sel] - g["a_rnn_states_out"][sel]).max() < TOL[precision]["h"]
    pool.close()


def test_unassigned_rows_untouched_and_bad_assignments(P, pkg):
    E = 150
    env, agents = make_env(pkg, "ppo", E)
    env.reset()
    nvec, n_shoot = heads(env.action_space)
    nh = len(nvec) + n_shoot
    rng = np.random.default_rng(3)
    h, m = random_inputs(env, agents, rng)
    pool = pool_for(P, env, "ppo", "fast", 4, seed=5)
    for k in range(3):
        pool.load_state_dict(k, member_sd(env.obs_dim, nvec, n_shoot, True, 700 + k))
    members = rng.integers(-1, 3, E).astype(np.int32)
    members[:3] = [-1, 2, -1]
    pool.assign(members)
    act_d = env.device_tensors()[0]
    act_d.fill_(-7.0)
    ho = torch.full_like(h, -5.0)
    lp = torch.full((E, 1), -3.0, device="cuda")
    pool.act_into_env(env, h, m, agents=agents, counter=0, rnn_states_out=ho, logp_out=lp)
    torch.cuda.current_stream().synchronize()
    un = torch.as_tensor(members < 0).cuda()
    assert (act_d[un] == -7.0).all() and (ho[un] == -5.0).all() and (lp[un] == -3.0).all()
    assert (act_d[~un][:, 0] == -7.0).all()                     # the learner's agent 0 is not this pool's
    assert (act_d[~un][:, 1, :nh] != -7.0).all() and (ho[~un] != -5.0).all() and (lp[~un] != -3.0).all()
    # out-of-range and unloaded members are named by assign(check=True); with check=False they are skipped like -1
    bad = members.copy()
    bad[17] = 9
    with pytest.raises(ValueError, match="env 17 has member 9, out of range"):
        pool.assign(bad)
    bad = members.copy()
    bad[40] = 3   # never loaded
    with pytest.raises(ValueError, match="env 40 has member 3, not loaded"):
        pool.assign(bad)
    pool.assign(bad, check=False)
    ho2 = torch.full_like(h, -5.0)
    pool.act_into_env(env, h, m, agents=agents, counter=0, rnn_states_out=ho2)
    torch.cuda.current_stream().synchronize()
    assert (ho2[40] == -5.0).all()
    keep = np.nonzero(bad >= 0)[0]
    keep = torch.as_tensor(keep[keep != 40]).cuda()
    assert torch.equal(ho2[keep], ho[keep])
    pool.close()
    env.close()


@pytest.mark.parametrize("precision", ["fast", "fp32"])
def test_load_paths_copy_from_and_reassign(P, pkg, precision):
    g = U.golden()
    obs_s, act_s = U.spaces("b")
    sd0, _ = U.state_dicts(g, "b")
    obs_dim, nvec = U.CASES["b"][:2]
    sd1 = member_sd(obs_dim, nvec, 0, True, 811)
    pool = P.DevicePolicyPool(obs_s, act_s, U.args("b"), 4, precision=precision, seed=9)
    learner = P.DevicePolicy(obs_s, act_s, U.args("b"), precision=precision, seed=9)   # with a critic: its actor is copied
    learner.load_state_dict(sd0, U.state_dicts(g, "b")[1])
    pool.load_state_dict(0, sd0)
    pool.load_from_torch(1, {k: torch.as_tensor(v).cuda() for k, v in sd0.items()})
    pool.copy_from(2, learner)
    assert torch.equal(pool.packed(0), learner.packed(0))
    assert torch.equal(pool.packed(1), pool.packed(0)) and torch.equal(pool.packed(2), pool.packed(0))
    # refused loads keep the member's weights
    pool.load_state_dict(3, sd1)
    before = pool.packed(3)
    bad = {k: torch.as_tensor(v).cuda() for k, v in sd1.items()}
    bad["rnn.gru.weight_hh_l0"][3, 5] = float("nan")
    with pytest.raises(ValueError, match="refused"):
        pool.load_from_torch(3, bad)
    with pytest.raises(RuntimeError, match="not finite"):
        pool.load_state_dict(3, {k: v.cpu().numpy() for k, v in bad.items()})
    if precision == "fast":
        big = {k: torch.as_tensor(v).cuda() for k, v in sd1.items()}
        big["act.mlp.fc.0.weight"][0, 0] = 70000.0
        with pytest.raises(ValueError, match="refused"):
            pool.load_from_torch(3, big)
        with pytest.raises(RuntimeError, match="65504"):
            pool.load_state_dict(3, {k: v.cpu().numpy() for k, v in big.items()})
    assert torch.equal(pool.packed(3), before)
    # a copy across precision or form is refused
    other = P.DevicePolicy(obs_s, act_s, U.args("b"), precision="fp32" if precision == "fast" else "fast", critic=False)
    other.load_state_dict(sd0)
    with pytest.raises(RuntimeError, match="precision"):
        pool.copy_from(0, other)
    # re-assigning between calls takes effect from the next call
    ref1 = P.DevicePolicy(obs_s, act_s, U.args("b"), precision=precision, seed=9, critic=False)
    ref1.load_state_dict(sd1)
    n = len(g["b_obs"])
    pool.assign(np.zeros(n, np.int32))
    a0, h0 = pool.act(g["b_obs"], g["b_rnn_states"], g["b_masks"], counter=4)
    want0 = learner.act(g["b_obs"], g["b_rnn_states"], g["b_masks"], counter=4)
    pool.assign(np.full(n, 3, np.int32))
    a1, h1 = pool.act(g["b_obs"], g["b_rnn_states"], g["b_masks"], counter=4)
    want1 = ref1.act(g["b_obs"], g["b_rnn_states"], g["b_masks"], counter=4)
    assert np.array_equal(a0, want0[0]) and np.array_equal(h0, want0[1])
    assert np.array_equal(a1, want1[0]) and np.array_equal(h1, want1[1])
    assert not np.array_equal(h0, h1)
    for p in (pool, learner, other, ref1):
        p.close()


@pytest.mark.parametrize("n", [1, 31, 33, 32768])
def test_sizes(P, n):
    g = U.golden()
    obs_s, act_s = U.spaces("a")
    obs_dim, nvec, n_shoot = U.CASES["a"][:3]
    sds = [U.state_dicts(g, "a")[0], member_sd(obs_dim, nvec, n_shoot, False, 901), member_sd(obs_dim, nvec, n_shoot, False, 902)]
    pool = P.DevicePolicyPool(obs_s, act_s, U.args("a"), 3, seed=2)
    for k, sd in enumerate(sds):
        pool.load_state_dict(k, sd)
    idx = np.arange(n) % len(g["a_obs"])
    obs = torch.as_tensor(g["a_obs"][idx].astype(np.float32)).cuda()
    h = torch.as_tensor(g["a_rnn_states"][idx]).cuda()
    m = torch.as_tensor(g["a_masks"][idx]).cuda()
    members = np.random.default_rng(n).integers(0, 3, n).astype(np.int32)
    pool.assign(members)
    a, ho, lp = pool.act(obs, h, m, counter=1, return_log_probs=True)
    for k, sd in enumerate(sds):
        ref = P.DevicePolicy(obs_s, act_s, U.args("a"), seed=2, critic=False)
        ref.load_state_dict(sd)
        ar, hr, lr = ref.act(obs, h, m, counter=1, return_log_probs=True)
        torch.cuda.current_stream().synchronize()
        sel = torch.as_tensor(members == k).cuda()
        assert torch.equal(a[sel], ar[sel]) and torch.equal(ho[sel], hr[sel]) and torch.equal(lp[sel], lr[sel]), f"member {k}"
        ref.close()
    pool.close()


def test_stream_ordering_against_torch(P):
    g = U.golden()
    obs_s, act_s = U.spaces("b")
    obs_dim, nvec = U.CASES["b"][:2]
    pool = P.DevicePolicyPool(obs_s, act_s, U.args("b"), 2)
    pool.load_state_dict(0, U.state_dicts(g, "b")[0])
    pool.load_state_dict(1, member_sd(obs_dim, nvec, 0, True, 955))
    n = 4096
    rng = np.random.default_rng(5)
    obs_np = rng.normal(0, 0.5, (n, obs_dim)).astype(np.float32)
    h_np = rng.normal(0, 0.5, (n, 1, 128)).astype(np.float32)
    pool.assign(rng.integers(0, 2, n).astype(np.int32))
    want = pool.act(obs_np, h_np, np.ones((n, 1), np.float32), deterministic=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        obs = torch.zeros(n, obs_dim, device="cuda")
        h = torch.zeros(n, 1, 128, device="cuda")
        torch.cuda._sleep(2_000_000)          # the copies below land well after the call is queued
        obs.copy_(torch.from_numpy(obs_np).cuda(non_blocking=True))
        h.copy_(torch.from_numpy(h_np).cuda(non_blocking=True))
        out = pool.act(obs, h, torch.ones(n, 1, device="cuda"), deterministic=True)
        acts = out[0] * 1.0                  # a torch consumer on the same stream
    s.synchronize()
    for x, y in zip(out, want):
        assert np.array_equal(x.cpu().numpy(), y)
    assert np.array_equal(acts.cpu().numpy(), want[0])
    pool.close()


def test_rollout_learner_and_pool_into_env(P, pkg):
    E = 64
    env, agents = make_env(pkg, "ppo", E, seed=13)
    ref, _ = make_env(pkg, "ppo", E, seed=13)
    nvec, n_shoot = heads(env.action_space)
    learner = single(P, env, "ppo", member_sd(env.obs_dim, nvec, n_shoot, True, 1001), "fast", 4)
    pool = pool_for(P, env, "ppo", "fast", 3, seed=8)
    for k in range(3):
        pool.load_state_dict(k, member_sd(env.obs_dim, nvec, n_shoot, True, 1010 + k))
    pool.assign_split(E, [2, 0, 1])
    env.reset()
    ref.reset()
    act_d = env.device_tensors()[0]
    hl, ho = torch.zeros(E, 1, 128, device="cuda"), torch.zeros(E, 1, 128, device="cuda")
    masks = torch.ones(E, 1, device="cuda")
    for step in range(10):
        learner.act_into_env(env, hl, masks, agents=slice(0, 1), counter=step)
        pool.act_into_env(env, ho, masks, agents=agents, counter=step)
        torch.cuda.current_stream().synchronize()
        dev_act = act_d.clone()
        env.step_device(stream=torch.cuda.current_stream())
        ref.step(dev_act.cpu().numpy())
        torch.cuda.current_stream().synchronize()
    env.sync()
    assert env.full_state_checksum() == ref.full_state_checksum()
    for p in (learner, pool):
        p.close()
    env.close()
    ref.close()
