"""The device PPO policy (DevicePolicy, csrc/policy_kernel.hpp) on the MI355X against tests/golden/policy_1v1.npz and policy_seeded.npz: the reference's own
actor / critic in float64 (tests/golden/make_policy_golden.py), the shipped 1v1_actor.pt and a seeded actor + critic."""
import importlib
import types

import numpy as np
import pytest

import policy_util as U

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# about 4x the worst errors measured against the float64 golden ("The PPO rollout policy": fast 5.1e-6 / 1.0e-6 / 1.6e-6, fp32
# 2.1e-6 / 5.1e-7 / 6.2e-7 for log-prob / GRU state / value); the fast form's log-prob bound is 3.9x
TOL = {"fast": {"logp": 2e-5, "h": 4.2e-6, "v": 6.5e-6}, "fp32": {"logp": 1e-5, "h": 2.1e-6, "v": 2.5e-6}}
MARGIN = 1e-4   # rows whose golden top-two logits (or |p - 0.5|) are this close may take either action


@pytest.fixture(scope="module")
def P(pkg):
    return importlib.import_module("aircombat-selfplay_amd.policy")


@pytest.fixture(scope="module")
def g():
    return U.golden()


def make(P, tag, precision, g, seed=0):
    obs, act = U.spaces(tag)
    asd, csd = U.state_dicts(g, tag)
    pol = P.DevicePolicy(obs, act, U.args(tag), precision=precision, seed=seed, critic=csd is not None)
    pol.load_state_dict(asd, csd)
    return pol


def cuda(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).cuda()


def ambiguous(g, tag):
    """[N, heads] True where the golden's action is within MARGIN of a tie."""
    nvec, n_shoot = U.CASES[tag][1], U.CASES[tag][2]
    lg, cols, off = g[f"{tag}_logits"], [], 0
    for n in nvec:
        s = np.sort(lg[:, off:off + n], -1)
        cols.append(s[:, -1] - s[:, -2] < MARGIN if n > 1 else np.zeros(len(lg), bool))
        off += n
    for k in range(n_shoot):
        cols.append(np.abs(g[f"{tag}_shoot_p"][:, k] - 0.5) < MARGIN)
    return np.stack(cols, -1)


def run(pol, g, tag, deterministic=True, counter=None):
    obs, h, m = cuda(g[f"{tag}_obs"]), cuda(g[f"{tag}_rnn_states"]), cuda(g[f"{tag}_masks"])
    if pol.has_critic:
        v, a, lp, ha, hc = pol.get_actions(obs, h, cuda(g[f"{tag}_rnn_states_critic"]), m, deterministic=deterministic, counter=counter)
    else:
        a, ha, lp = pol.act(obs, h, m, deterministic=deterministic, counter=counter, return_log_probs=True)
        v = hc = None
    torch.cuda.current_stream().synchronize()
    f = lambda t: None if t is None else t.double().cpu().numpy()
    return f(v), f(a), f(lp), f(ha), f(hc)


@pytest.mark.parametrize("precision", ["fast", "fp32"])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_golden_deterministic(P, g, tag, precision):
    pol = make(P, tag, precision, g)
    v, a, lp, ha, hc = run(pol, g, tag)
    amb = ambiguous(g, tag)
    ok = (a == g[f"{tag}_actions"]) | amb
    assert ok.all(), f"{(~ok).sum()} actions differ outside tie margins"
    exact = (a == g[f"{tag}_actions"]).all(-1)   # the log-prob is compared where every head took the golden's action
    e_lp = np.abs(lp - g[f"{tag}_log_probs"])[exact].max()
    e_h = np.abs(ha - g[f"{tag}_rnn_states_out"]).max()
    print(f"\n[{tag} {precision}] max |d logp| {e_lp:.3g}  |d h| {e_h:.3g}  rows with a tie-flipped head {int((~exact).sum())}", end="")
    assert e_lp < TOL[precision]["logp"]
    assert e_h < TOL[precision]["h"]
    if v is not None:
        e_v = np.abs(v - g[f"{tag}_values"]).max()
        e_hc = np.abs(hc - g[f"{tag}_rnn_states_critic_out"]).max()
        print(f"  |d v| {e_v:.3g}  |d hc| {e_hc:.3g}", end="")
        assert e_v < TOL[precision]["v"]
        assert e_hc < TOL[precision]["h"]
    pol.close()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_stochastic_matches_inverse_cdf(P, g, tag):
    pol = make(P, tag, "fast", g, seed=1234)
    nvec, n_shoot = U.CASES[tag][1], U.CASES[tag][2]
    n = len(g[f"{tag}_obs"])
    excused = np.zeros(n, bool)
    for counter in (0, 9):
        _, a, lp, _, _ = run(pol, g, tag, deterministic=False, counter=counter)
        want_lp = np.zeros(n)
        off = 0
        for h, k in enumerate(nvec):
            u = P.draw_host(1234, counter, n, h).astype(np.float64)
            pr = g[f"{tag}_probs"][:, off:off + k]
            pick, edge = U.inverse_cdf(pr, u)
            excused |= edge < 1e-5
            ok = (a[:, h] == pick) | excused
            assert ok.all(), f"head {h}: {(~ok).sum()} picks differ"
            want_lp += np.log(pr[np.arange(n), pick])
            off += k
        for s in range(n_shoot):
            u = P.draw_host(1234, counter, n, len(nvec) + s).astype(np.float64)
            p = g[f"{tag}_shoot_p"][:, s]
            fire = (u >= 1.0 - p).astype(np.float64)
            excused |= np.abs(u - (1.0 - p)) < 1e-5
            ok = (a[:, len(nvec) + s] == fire) | excused
            assert ok.all(), f"munition head {s}: {(~ok).sum()} differ"
            want_lp += np.where(fire > 0, np.log(p), np.log1p(-p))
        assert np.abs(lp[:, 0] - want_lp)[~excused].max() < 1e-4
        # the draws do move the actions: a different counter gives different picks
        if counter == 0:
            a0 = a
    assert (a0 != a).any()
    assert pol.counter == 0   # explicit counters do not advance the policy's own
    pol.close()


def test_zero_mask_equals_zero_state(P, g):
    pol = make(P, "b", "fast", g)
    obs = cuda(g["b_obs"][:64])
    h, hc = cuda(g["b_rnn_states"][:64]), cuda(g["b_rnn_states_critic"][:64])
    zero = torch.zeros_like(h)
    r1 = pol.get_actions(obs, h, hc, torch.zeros(64, 1).cuda(), deterministic=True)
    r2 = pol.get_actions(obs, zero, zero, torch.ones(64, 1).cuda(), deterministic=True)
    torch.cuda.current_stream().synchronize()
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)
    pol.close()


@pytest.mark.parametrize("precision", ["fast", "fp32"])
def test_load_device_matches_host_and_refusals_keep_weights(P, g, precision):
    asd, csd = U.state_dicts(g, "b")
    host = make(P, "b", precision, g)
    obs, act = U.spaces("b")
    dev = P.DevicePolicy(obs, act, U.args("b"), precision=precision)
    ta = {k: torch.as_tensor(v).cuda() for k, v in asd.items()}
    tc = {k: torch.as_tensor(v).cuda() for k, v in csd.items()}
    dev.load_from_torch(ta, tc)
    for net in (0, 1):
        assert torch.equal(dev.packed(net), host.packed(net)), f"net {net}"
    before = [dev.packed(0), dev.packed(1)]
    bad = dict(ta)
    bad["rnn.gru.weight_hh_l0"] = ta["rnn.gru.weight_hh_l0"].clone()
    bad["rnn.gru.weight_hh_l0"][3, 5] = float("nan")
    with pytest.raises(ValueError, match="refused"):
        dev.load_from_torch(bad, tc)
    with pytest.raises(RuntimeError, match="not finite"):
        dev.load_state_dict({k: v.cpu() for k, v in bad.items()}, csd)
    big = dict(ta)
    big["act.mlp.fc.0.weight"] = ta["act.mlp.fc.0.weight"].clone()
    big["act.mlp.fc.0.weight"][0, 0] = 70000.0
    if precision == "fast":
        with pytest.raises(ValueError, match="refused"):
            dev.load_from_torch(big, tc)
        with pytest.raises(RuntimeError, match="65504"):
            dev.load_state_dict({k: v.cpu() for k, v in big.items()}, csd)
    assert torch.equal(dev.packed(0), before[0]) and torch.equal(dev.packed(1), before[1])
    if precision == "fp32":   # the reference-precision form takes any finite weight
        dev.load_from_torch(big, tc)
        assert not torch.equal(dev.packed(0), before[0])
    host.close()
    dev.close()


def test_stream_ordering_against_torch(P, g):
    pol = make(P, "b", "fast", g)
    n = 4096
    rng = np.random.default_rng(5)
    obs_np = rng.normal(0, 0.5, (n, 15)).astype(np.float32)
    h_np = rng.normal(0, 0.5, (n, 1, 128)).astype(np.float32)
    want = pol.get_actions(obs_np, h_np, h_np, np.ones((n, 1), np.float32), deterministic=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        obs = torch.zeros(n, 15, device="cuda")
        h = torch.zeros(n, 1, 128, device="cuda")
        torch.cuda._sleep(2_000_000)          # the copies below land well after the call is queued
        obs.copy_(torch.from_numpy(obs_np).cuda(non_blocking=True))
        h.copy_(torch.from_numpy(h_np).cuda(non_blocking=True))
        out = pol.get_actions(obs, h, h, torch.ones(n, 1, device="cuda"), deterministic=True)
        vals = out[0] * 1.0                  # a torch consumer on the same stream
    s.synchronize()
    for x, y in zip(out, want):
        assert np.array_equal(x.cpu().numpy(), y)
    assert np.array_equal(vals.cpu().numpy(), want[0])
    pol.close()


def _random_sd(P, cfg, rng, critic):
    keys = P.blob_keys(cfg)[1 if critic else 0]
    shapes = {}
    D = cfg.obs_dim
    for k in keys:
        if "feature_norm" in k:
            shapes[k] = (D,)
        elif k.endswith("fc.0.weight") and k.startswith("base."):
            shapes[k] = (128, D)
        elif "gru.weight" in k:
            shapes[k] = (384, 128)
        elif "gru.bias" in k:
            shapes[k] = (384,)
        elif "logits_net.weight" in k:
            shapes[k] = (cfg.nvec[int(k.split(".")[2])], 128)
        elif "logits_net.bias" in k:
            shapes[k] = (cfg.nvec[int(k.split(".")[2])],)
        elif k.endswith("weight") and (".fc.0." in k or ".fc.3." in k):
            shapes[k] = (128, 128)
        elif k == "value_out.weight":
            shapes[k] = (1, 128)
        elif k == "value_out.bias":
            shapes[k] = (1,)
        else:
            shapes[k] = (128,)
    return {k: (rng.normal(0, 0.15, s) + (1.0 if k.endswith(("fc.2.weight", "fc.5.weight", "norm.weight")) else 0.0)).astype(np.float32)
            for k, s in shapes.items()}


def test_selfplay_agents_into_env_and_step_device(P, pkg):
    cfg = pkg.default_nvn_config(2)
    env = pkg.HipVecEnv(cfg, 64, device_id=0, seed=3)
    ref = pkg.HipVecEnv(cfg, 64, device_id=0, seed=3)
    E, A = env.num_envs, env.num_agents
    assert A == 4
    args = types.SimpleNamespace(hidden_size="128 128", act_hidden_size="128 128", recurrent_hidden_size=128, recurrent_hidden_layers=1,
                                 activation_id=1, use_feature_normalization=True, use_prior=False, use_recurrent_policy=True)
    rng = np.random.default_rng(8)
    pols = []
    for _ in range(2):
        p = P.DevicePolicy(env.observation_space, env.action_space, args, seed=int(rng.integers(1 << 30)), critic=False)
        p.load_state_dict(_random_sd(P, p.cfg, rng, False))
        pols.append(p)
    obs0 = env.reset()
    ref.reset()
    act_d, obs_d, _, _, _ = env.device_tensors()
    hs = [torch.zeros(E * 2, 1, 128, device="cuda") for _ in range(2)]
    masks = torch.ones(E * 2, 1, device="cuda")
    obs_prev = torch.as_tensor(obs0).cuda()
    for step in range(10):
        h_before = [h.clone() for h in hs]
        for k, (p, h) in enumerate(zip(pols, hs)):
            p.act_into_env(env, h, masks, agents=slice(2 * k, 2 * k + 2), counter=step)
        # the same actions computed separately, from the observation the env holds
        sep = [pols[k].act(obs_prev[:, 2 * k:2 * k + 2].reshape(-1, env.obs_dim), h_before[k], masks, counter=step)[0] for k in range(2)]
        torch.cuda.current_stream().synchronize()
        dev_act = act_d.clone()
        for k in range(2):
            assert torch.equal(dev_act[:, 2 * k:2 * k + 2, :4].reshape(-1, 4), sep[k]), f"step {step} team {k}"
        env.step_device(stream=torch.cuda.current_stream())
        ref.step(dev_act.cpu().numpy())
        torch.cuda.current_stream().synchronize()
        obs_prev = obs_d.clone()
    env.sync()
    assert env.full_state_checksum() == ref.full_state_checksum()
    for p in pols:
        p.close()
    env.close()
    ref.close()


@pytest.mark.parametrize("n", [1, 31, 33, 32768])
def test_sizes(P, g, n):
    pol = make(P, "a", "fast", g)
    idx = np.arange(n) % len(g["a_obs"])
    obs, h, m = cuda(g["a_obs"][idx]), cuda(g["a_rnn_states"][idx]), cuda(g["a_masks"][idx])
    sentinel = torch.full((n + 8, 7), -7.0, device="cuda")
    a, ha = pol.act(obs, h, m, deterministic=True)
    torch.cuda.current_stream().synchronize()
    amb = ambiguous(g, "a")[idx]
    assert ((a.double().cpu().numpy() == g["a_actions"][idx]) | amb).all()
    assert np.abs(ha.double().cpu().numpy() - g["a_rnn_states_out"][idx]).max() < TOL["fast"]["h"]
    # rows past n are never written: an agent range writing into a larger buffer leaves the rest alone
    rows = P.AcPolicyRows(n, 1, 1, 0, 7)
    lp = torch.empty(n, 1, device="cuda")
    ho = torch.empty(n, 1, 128, device="cuda")
    pol._launch(rows, obs, h, None, m, True, None, sentinel, lp, ho, None, 0)
    torch.cuda.current_stream().synchronize()
    assert torch.equal(sentinel[:n], a)
    assert (sentinel[n:] == -7.0).all()
    pol.close()
