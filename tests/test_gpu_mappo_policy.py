"""The device MAPPO policy (DeviceMAPPOPolicy: csrc/policy_kernel.hpp's wide form) on the MI355X against tests/golden/mappo_{a,b,c,d}.npz,
the reference's own MAPPO actor / critic in float64 (tests/golden/make_mappo_golden.py); get_values; the env-share critic input against
explicit cent_obs; a rollout into DeviceSharedReplayBuffer; and DevicePolicy.get_values."""
import importlib
import types

import numpy as np
import pytest

import mappo_util as M
import policy_util as U

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# about 4x the worst errors measured against the float64 golden over cases a-d ("The PPO rollout policy": fast 4.7e-6 /
# 1.9e-6 / 4.4e-6, fp32 1.7e-6 / 4.8e-7 / 7.5e-7 for log-prob / GRU state (actor or critic) / value)
TOL = {"fast": {"logp": 2e-5, "h": 7.5e-6, "v": 1.75e-5}, "fp32": {"logp": 6.6e-6, "h": 1.9e-6, "v": 3e-6}}
MARGIN = 1e-4
TAGS = ["a", "b", "c", "d"]


@pytest.fixture(scope="module")
def P(pkg):
    return importlib.import_module("aircombat-selfplay_amd.policy")


@pytest.fixture(scope="module")
def goldens():
    return {t: M.golden_case(t) for t in TAGS}


def cuda(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).cuda()


def make(P, tag, precision, g, seed=0, critic=True):
    o, c, act = M.spaces(tag)
    pol = P.DeviceMAPPOPolicy(o, c, act, M.args(tag), precision=precision, seed=seed, critic=critic)
    pol.load_state_dict(g["sd"], g["critic_sd"] if critic else None)
    return pol


def ambiguous(g, tag):
    nvec, n_shoot = M.CASES[tag][3], M.CASES[tag][4]
    cols, off = [], 0
    for n in nvec:
        s = np.sort(g["logits"][:, off:off + n], -1)
        cols.append(s[:, -1] - s[:, -2] < MARGIN)
        off += n
    for k in range(n_shoot):
        cols.append(np.abs(g["shoot_p"][:, k] - 0.5) < MARGIN)
    return np.stack(cols, -1)


def run(pol, g, deterministic=True, counter=None):
    out = pol.get_actions(cuda(g["cent_obs"]), cuda(g["obs"]), cuda(g["rnn_states"]), cuda(g["rnn_states_critic"]), cuda(g["masks"]),
                          deterministic=deterministic, counter=counter)
    torch.cuda.current_stream().synchronize()
    return [t.double().cpu().numpy() for t in out]


@pytest.mark.parametrize("precision", ["fast", "fp32"])
@pytest.mark.parametrize("tag", TAGS)
def test_golden_deterministic(P, goldens, tag, precision):
    g = goldens[tag]
    pol = make(P, tag, precision, g)
    v, a, lp, ha, hc = run(pol, g)
    ok = (a == g["actions"]) | ambiguous(g, tag)
    assert ok.all(), f"{(~ok).sum()} actions differ outside tie margins"
    exact = (a == g["actions"]).all(-1)
    e_lp = np.abs(lp - g["log_probs"])[exact].max()
    e_h = np.abs(ha - g["rnn_states_out"]).max()
    e_v = np.abs(v - g["values"]).max()
    e_hc = np.abs(hc - g["rnn_states_critic_out"]).max()
    print(f"\n[{tag} {precision}] max |d logp| {e_lp:.3g}  |d h| {e_h:.3g}  |d v| {e_v:.3g}  |d hc| {e_hc:.3g}  "
          f"tie rows {int((~exact).sum())}", end="")
    assert e_lp < TOL[precision]["logp"]
    assert e_h < TOL[precision]["h"] and e_hc < TOL[precision]["h"]
    assert e_v < TOL[precision]["v"]
    # get_values: critic workgroups only, the same values bit for bit
    vv = pol.get_values(cuda(g["cent_obs"]), cuda(g["rnn_states_critic"]), cuda(g["masks"]))
    assert np.array_equal(vv.double().cpu().numpy(), v)
    # the actor-only form (a self-play opponent): the same actions and states as the full call
    opp = make(P, tag, precision, g, critic=False)
    a2, ha2, lp2 = opp.act(cuda(g["obs"]), cuda(g["rnn_states"]), cuda(g["masks"]), deterministic=True, return_log_probs=True)
    assert np.array_equal(a2.double().cpu().numpy(), a) and np.array_equal(ha2.double().cpu().numpy(), ha)
    assert np.array_equal(lp2.double().cpu().numpy(), lp)
    pol.close()
    opp.close()


def test_devicepolicy_get_values_against_golden(P):
    g = U.golden()
    obs, act = U.spaces("b")
    asd, csd = U.state_dicts(g, "b")
    for precision in ("fast", "fp32"):
        pol = P.DevicePolicy(obs, act, U.args("b"), precision=precision)
        pol.load_state_dict(asd, csd)
        o, hc, m = cuda(g["b_obs"]), cuda(g["b_rnn_states_critic"]), cuda(g["b_masks"])
        v = pol.get_values(o, hc, m)
        full = pol.get_actions(o, cuda(g["b_rnn_states"]), hc, m, deterministic=True)[0]
        torch.cuda.current_stream().synchronize()
        assert torch.equal(v, full)
        assert np.abs(v.double().cpu().numpy() - g["b_values"]).max() < TOL[precision]["v"]
        vn = pol.get_values(g["b_obs"], g["b_rnn_states_critic"], g["b_masks"])   # numpy in, numpy out
        assert isinstance(vn, np.ndarray) and np.array_equal(vn, v.cpu().numpy())
        pol.close()


@pytest.mark.parametrize("precision", ["fast", "fp32"])
def test_load_paths_identical_and_refusals_keep_weights(P, goldens, precision):
    g = goldens["b"]
    host = make(P, "b", precision, g)
    o, c, act = M.spaces("b")
    dev = P.DeviceMAPPOPolicy(o, c, act, M.args("b"), precision=precision)
    ta = {k: torch.as_tensor(v).cuda() for k, v in g["sd"].items()}
    tc = {k: torch.as_tensor(v).cuda() for k, v in g["critic_sd"].items()}
    dev.load_from_torch(ta, tc)
    for net in (0, 1):
        assert torch.equal(dev.packed(net), host.packed(net)), f"net {net}"
    before = [dev.packed(0), dev.packed(1)]
    bad = dict(tc)
    bad["base.mlp.fc.0.weight"] = tc["base.mlp.fc.0.weight"].clone()
    bad["base.mlp.fc.0.weight"][7, 500] = float("inf")     # in the last K-block of the 520-wide layer 1
    with pytest.raises(ValueError, match="refused"):
        dev.load_from_torch(ta, bad)
    with pytest.raises(RuntimeError, match="not finite"):
        dev.load_state_dict(g["sd"], {k: v.cpu() for k, v in bad.items()})
    if precision == "fast":
        big = dict(tc)
        big["base.feature_norm.weight"] = tc["base.feature_norm.weight"].clone()
        big["base.feature_norm.weight"][519] = 1e5
        with pytest.raises(ValueError, match="refused"):
            dev.load_from_torch(ta, big)
        with pytest.raises(RuntimeError, match="65504"):
            dev.load_state_dict(g["sd"], {k: v.cpu() for k, v in big.items()})
    assert torch.equal(dev.packed(0), before[0]) and torch.equal(dev.packed(1), before[1])
    # the weights in place still compute the golden
    v, a, lp, ha, hc = run(dev, g)
    assert np.abs(v - g["values"]).max() < TOL[precision]["v"]
    host.close()
    dev.close()


@pytest.mark.parametrize("n,na", [(1, 1), (31, 1), (33, 3), (32768, 4), (96, 3), (35, 5)])
def test_partial_tiles_and_agent_ranges(P, goldens, n, na):
    g = goldens["a"]
    pol = make(P, "a", "fast", g)
    idx = np.arange(n) % 256
    obs, co = cuda(g["obs"][idx]), cuda(g["cent_obs"][idx])
    h, hc, m = cuda(g["rnn_states"][idx]), cuda(g["rnn_states_critic"][idx]), cuda(g["masks"][idx])
    v, a, lp, ha, hco = pol.get_actions(co, obs, h, hc, m, deterministic=True)
    torch.cuda.current_stream().synchronize()
    amb = ambiguous(g, "a")[idx]
    assert ((a.double().cpu().numpy() == g["actions"][idx]) | amb).all()
    assert np.abs(v.double().cpu().numpy() - g["values"][idx]).max() < TOL["fast"]["v"]
    assert np.abs(hco.double().cpu().numpy() - g["rnn_states_critic_out"][idx]).max() < TOL["fast"]["h"]
    # an agent range [1, 1 + na) of A = na + 2 writes only its own action rows; rows past it stay untouched
    A, E = na + 2, n // na
    if E * na == n and E > 0:
        nr = E * na
        obs_b = torch.zeros(E, A, 39, device="cuda")
        obs_b[:, 1:1 + na] = obs[:nr].reshape(E, na, 39)
        sentinel = torch.full((E * A + 8, 7), -7.0, device="cuda")
        rows = P.AcPolicyRows(nr, na, A, 1, 7)
        vals, lp2 = torch.empty(nr, 1, device="cuda"), torch.empty(nr, 1, device="cuda")
        ho, hco2 = torch.empty(nr, 1, 128, device="cuda"), torch.empty(nr, 1, 128, device="cuda")
        pol._launch(rows, obs_b, h[:nr], hc[:nr], m[:nr], True, vals, sentinel, lp2, ho, hco2, 0, cin=co[:nr].contiguous())
        torch.cuda.current_stream().synchronize()
        got = sentinel[:E * A].reshape(E, A, 7)
        assert torch.equal(got[:, 1:1 + na].reshape(nr, 7), a[:nr])
        assert (got[:, 0] == -7.0).all() and (got[:, 1 + na:] == -7.0).all() and (sentinel[E * A:] == -7.0).all()
        assert torch.equal(vals, v[:nr]) and torch.equal(ho, ha[:nr]) and torch.equal(hco2, hco[:nr])
    pol.close()


def _nvn_policies(P, env, rng):
    """A learner (MAPPO: actor + critic on share_obs) and an actor-only opponent for a 2v2 env, random weights."""
    o, act = env.observation_space, env.action_space
    cent = env.share_observation_space
    args = types.SimpleNamespace(hidden_size="128 128", act_hidden_size="128 128", recurrent_hidden_size=128, recurrent_hidden_layers=1,
                                 activation_id=1, use_feature_normalization=True, use_prior=True, use_recurrent_policy=True)
    learner = P.DeviceMAPPOPolicy(o, cent, act, args, seed=int(rng.integers(1 << 30)))
    opp = P.DeviceMAPPOPolicy(o, cent, act, args, seed=int(rng.integers(1 << 30)), critic=False)

    def sd(D, critic, scale):
        keys = P.blob_keys(learner.cfg)[1 if critic else 0]
        out = {}
        for k in keys:
            if "feature_norm" in k:
                s = (D,)
            elif k == "base.mlp.fc.0.weight":
                s = (128, D)
            elif "gru.weight" in k:
                s = (384, 128)
            elif "gru.bias" in k:
                s = (384,)
            elif "logits_net" in k or ".net." in k:
                h = int(k.split(".")[2])
                w = learner.cfg.nvec[h] if h < learner.cfg.n_cat else 2
                s = (w, 128) if k.endswith("weight") else (w,)
            elif k.endswith("weight") and (".fc.0." in k or ".fc.3." in k):
                s = (128, 128)
            elif k == "value_out.weight":
                s = (1, 128)
            elif k == "value_out.bias":
                s = (1,)
            else:
                s = (128,)
            out[k] = (rng.normal(0, scale, s) + (1.0 if k.endswith(("fc.2.weight", "fc.5.weight", "norm.weight")) else 0.0)).astype(np.float32)
        return out

    learner.load_state_dict(sd(env.obs_dim, False, 0.15), sd(cent.shape[0], True, 0.1))
    opp.load_state_dict(sd(env.obs_dim, False, 0.15))
    return learner, opp


def test_env_share_equals_explicit_with_selfplay_opponent(P, pkg):
    cfg = pkg.default_config("scenario2_nvn")
    env = pkg.HipShareVecEnv(cfg, 48, device_id=0, seed=5)
    E, A, D = env.num_envs, env.num_agents, env.obs_dim
    assert (A, D) == (4, 39) and env.share_observation_space.shape == (156,)
    rng = np.random.default_rng(21)
    learner, opp = _nvn_policies(P, env, rng)
    env.reset()
    act_d, obs_d, _, _, _ = env.device_tensors()
    n = E * 2
    ha, hc, ho = (torch.zeros(n, 1, 128, device="cuda") for _ in range(3))
    ha_x, hc_x, ho_x = ha.clone(), hc.clone(), ho.clone()
    masks = torch.ones(n, 1, device="cuda")
    for step in range(4):
        obs_now = obs_d.clone()
        vals, lp, _, _ = learner.get_actions_into_env(env, ha, hc, masks, agents=slice(0, 2), counter=step)
        opp.act_into_env(env, ho, masks, agents=slice(2, 4), counter=step)
        # explicit: share_obs built by torch from the env's obs view, the same counters
        share = obs_now.reshape(E, 1, A * D).expand(E, A, A * D)
        v_x, a_x, lp_x, ha_x, hc_x = learner.get_actions(share[:, :2].reshape(n, A * D), obs_now[:, :2].reshape(n, D), ha_x, hc_x, masks,
                                                         counter=step)
        ao_x, ho_x = opp.act(obs_now[:, 2:].reshape(n, D), ho_x, masks, counter=step)
        vg = learner.get_values_from_env(env, hc, masks, agents=slice(0, 2))
        vg_x = learner.get_values(share[:, :2].reshape(n, A * D), hc_x, masks)
        torch.cuda.current_stream().synchronize()
        dev_act = act_d.clone()
        assert torch.equal(vals, v_x) and torch.equal(lp, lp_x), f"step {step}"
        assert torch.equal(ha, ha_x) and torch.equal(hc, hc_x) and torch.equal(ho, ho_x)
        nh = learner.n_heads
        assert torch.equal(dev_act[:, :2, :nh].reshape(n, nh), a_x) and torch.equal(dev_act[:, 2:, :nh].reshape(n, nh), ao_x)
        assert torch.equal(vg, vg_x)
        env.step_device(stream=torch.cuda.current_stream())
    # a cent_obs_space that is not num_agents * obs_dim wide is refused for the env-share input
    o, act = env.observation_space, env.action_space
    narrow = P.DeviceMAPPOPolicy(o, pkg.vec_env._Box(-10, 10, (2 * D,)), act, M.args("a"))
    with pytest.raises(P.UnsupportedPolicy, match="cent_obs_space"):
        narrow.get_actions_into_env(env, ha, hc, masks, agents=slice(0, 2))
    for p in (learner, opp, narrow):
        p.close()
    env.close()


def test_rollout_into_shared_buffer_matches_explicit(P, pkg):
    cfg = pkg.default_config("scenario2_nvn")
    E, T = 16, 3
    env = pkg.HipShareVecEnv(cfg, E, device_id=0, seed=9)
    A, D = env.num_agents, env.obs_dim
    rng = np.random.default_rng(4)
    learner, opp = _nvn_policies(P, env, rng)
    args = types.SimpleNamespace(buffer_size=T, gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False,
                                 recurrent_hidden_size=128, recurrent_hidden_layers=1, data_chunk_length=T, n_rollout_threads=E)
    buf = pkg.DeviceSharedReplayBuffer(args, 2, env.observation_space, env.share_observation_space, env.action_space)
    obs, share = env.reset()
    act_d, obs_d, rew_d, done_d, _ = env.device_tensors()
    n = E * 2
    ha, hc, ho = (torch.zeros(n, 1, 128, device="cuda") for _ in range(3))
    masks = torch.ones(n, 1, device="cuda")
    want_v, want_hc = [], []
    ha_x, hc_x = ha.clone(), hc.clone()
    for t in range(T):
        obs_now = obs_d.clone()
        vals, lp, ha_new, hc_new = learner.get_actions_into_env(env, ha, hc, masks, agents=slice(0, 2), counter=t,
                                                                rnn_states_actor_out=torch.empty_like(ha),
                                                                rnn_states_critic_out=torch.empty_like(hc))
        opp.act_into_env(env, ho, masks, agents=slice(2, 4), counter=t)
        share_x = obs_now.reshape(E, 1, A * D).expand(E, 2, A * D).reshape(n, A * D)
        v_x, _, _, ha_x, hc_x = learner.get_actions(share_x, obs_now[:, :2].reshape(n, D), ha_x, hc_x, masks, counter=t)
        want_v.append(v_x.cpu().numpy().reshape(E, 2, 1))
        want_hc.append(hc_x.cpu().numpy().reshape(E, 2, 1, 128))
        nh = learner.n_heads
        actions = act_d[:, :2, :nh].clone()
        env.step_device(stream=torch.cuda.current_stream())
        share_next = obs_d.reshape(E, 1, A * D).expand(E, 2, A * D).contiguous()
        buf.insert(obs_d[:, :2].contiguous(), share_next, actions, rew_d[:, :2].contiguous(), masks.reshape(E, 2, 1),
                   lp.reshape(E, 2, 1).expand(E, 2, nh).contiguous(), vals.reshape(E, 2, 1), ha_new.reshape(E, 2, 1, 128),
                   hc_new.reshape(E, 2, 1, 128), on_device=True)
        torch.cuda.current_stream().synchronize()
        ha, hc = ha_new, hc_new
    for t in range(T):
        assert np.array_equal(buf.array("value_preds")[t], want_v[t]), f"values, step {t}"
        assert np.array_equal(buf.array("rnn_states_critic")[t + 1], want_hc[t]), f"critic state, step {t}"
    for p in (learner, opp):
        p.close()
    buf.close()
    env.close()


def test_stream_ordering_against_torch(P, goldens):
    g = goldens["b"]
    pol = make(P, "b", "fast", g)
    idx = np.arange(4096) % 256
    args = [g["cent_obs"][idx], g["obs"][idx], g["rnn_states"][idx], g["rnn_states_critic"][idx], g["masks"][idx]]
    want = pol.get_actions(*args, deterministic=True)
    want_v = pol.get_values(args[0], args[3], args[4])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ts = [torch.zeros(np.asarray(x).shape, device="cuda") for x in args]
        torch.cuda._sleep(2_000_000)          # the copies below land well after the calls are queued
        for t, x in zip(ts, args):
            t.copy_(torch.from_numpy(np.asarray(x, dtype=np.float32)).cuda(non_blocking=True))
        out = pol.get_actions(*ts, deterministic=True)
        v = pol.get_values(ts[0], ts[3], ts[4])
        vals = out[0] * 1.0
    s.synchronize()
    for x, y in zip(out, want):
        assert np.array_equal(x.cpu().numpy(), y)
    assert np.array_equal(vals.cpu().numpy(), want[0]) and np.array_equal(v.cpu().numpy(), want_v)
    pol.close()
