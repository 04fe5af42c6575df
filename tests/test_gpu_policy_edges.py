"""The rollout policy kernels (csrc/policy_kernel.hpp: policy_kernel, policy_values_kernel, policy_wide_kernel and the two pool kernels)
on the MI355X at the edges of the configurations they accept, against the float64 restatement: every entry of
tests/policy_edges_util.py's table in both precisions, deterministic and stochastic, 250 rows each (a ragged last tile in every launch);
get_values and the actor-only form bit for bit; a pool of two members per form at an edge configuration. The comparison itself is
policy_edges_util.compare, which test_policy_edges_host.py shows able to fail. The bounds are test_gpu_policy.TOL /
test_gpu_mappo_policy.TOL, unchanged but for the log-prob's growth with the number and scale of the heads."""
import importlib
import types

import numpy as np
import pytest

import policy_edges_util as E
from test_gpu_mappo_policy import TOL as TOL_WIDE
from test_gpu_policy import TOL as TOL_PPO

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = {"ppo": TOL_PPO, "mappo": TOL_WIDE}
SEED = 1234
COUNTERS = {None: (0, 9), "ties": (0, 9), "sharp": (0, 9, 17, 31)}


@pytest.fixture(scope="module")
def P(pkg):
    return importlib.import_module("aircombat-selfplay_amd.policy")


def cuda(x):
    return torch.as_tensor(np.array(x, dtype=np.float32)).cuda()   # (a copy: the table's arrays are read-only)


def spaces(e, nvec=None):
    ve = importlib.import_module("aircombat-selfplay_amd.vec_env")
    act = ve._MultiDiscrete(nvec or e.nvec)
    act = ve._Tuple([act, ve._MultiDiscrete([2] * 4)]) if e.n_shoot else act
    return ve._Box(-10, 10, (e.obs_dim,)), (ve._Box(-10, 10, (e.cent,)) if e.form == "mappo" else None), act


def args(e):
    return types.SimpleNamespace(hidden_size="128 128", act_hidden_size="128 128", recurrent_hidden_size=128, recurrent_hidden_layers=1,
                                 activation_id=1, use_feature_normalization=e.fn, use_prior=e.n_shoot > 0, use_recurrent_policy=True)


def make(P, e, precision, sd, csd, nvec=None):
    o, c, act = spaces(e, nvec)
    if e.form == "ppo":
        pol = P.DevicePolicy(o, act, args(e), precision=precision, seed=SEED, critic=csd is not None)
    else:
        pol = P.DeviceMAPPOPolicy(o, c, act, args(e), precision=precision, seed=SEED, critic=csd is not None)
    pol.load_state_dict(sd, csd)
    return pol


def get_actions(pol, e, t, deterministic, counter=None):
    lead = (t["cent_obs"],) if e.form == "mappo" else ()
    out = pol.get_actions(*lead, t["obs"], t["rnn_states"], t["rnn_states_critic"], t["masks"], deterministic=deterministic, counter=counter)
    torch.cuda.current_stream().synchronize()
    return out


def f64(t):
    return t.double().cpu().numpy()


@pytest.mark.parametrize("precision", ["fast", "fp32"])
@pytest.mark.parametrize("name", E.NAMES)
def test_edge_configuration(P, name, precision):
    e, d, ref = E.ENTRIES[name], E.inputs(name), E.reference(name)
    t = {k: cuda(d[k]) for k in ("obs", "cent_obs", "rnn_states", "rnn_states_critic", "masks") if k in d}
    nh = len(e.nvec) + e.n_shoot
    pol = make(P, e, precision, d["sd"], d["critic_sd"])
    opp = make(P, e, precision, d["sd"], None)   # the actor-only form, as a self-play opponent runs it
    # ---- deterministic
    det = get_actions(pol, e, t, True, 0)
    dev = dict(zip(("v", "a", "lp", "ha", "hc"), (f64(x) for x in det)))
    # get_values (critic workgroups only) and act (no critic): the same bits as get_actions
    vv = pol.get_values(t["cent_obs"] if e.form == "mappo" else t["obs"], t["rnn_states_critic"], t["masks"])
    a2, ha2, lp2 = opp.act(t["obs"], t["rnn_states"], t["masks"], deterministic=True, counter=0, return_log_probs=True)
    torch.cuda.current_stream().synchronize()
    assert torch.equal(vv, det[0])
    assert torch.equal(a2, det[1]) and torch.equal(lp2, det[2]) and torch.equal(ha2, det[3])
    if e.derived == "ties":   # the zero head's own log-prob, by difference to the same call with that head of size 1
        sd1, nvec1 = E.one_head(d["sd"], e.nvec, E.ZERO_HEAD)
        one = make(P, e, precision, sd1, None, nvec=nvec1)
        a1, _, lp1 = one.act(t["obs"], t["rnn_states"], t["masks"], deterministic=True, return_log_probs=True)
        torch.cuda.current_stream().synchronize()
        dev["a_one"], dev["lp_one"] = f64(a1), f64(lp1)
        one.close()
    # ---- stochastic: the kernel's draws recomputed on the host, picks by inverse CDF of the restatement's probabilities
    dev["stoch"] = []
    for counter in COUNTERS[e.derived]:
        out = get_actions(pol, e, t, False, counter)
        u = np.stack([P.draw_host(SEED, counter, E.N, h) for h in range(nh)], -1)
        dev["stoch"].append({"u": u, "a": f64(out[1]), "lp": f64(out[2])})
    assert (dev["stoch"][0]["a"] != dev["stoch"][1]["a"]).any() or all(k == 1 for k in e.nvec)   # the draws do move the actions
    assert pol.counter == 0   # explicit counters do not advance the policy's own
    # rows past the last are never written: the actor-only launch into larger buffers of sentinels, the same call otherwise
    sent_a = torch.full((E.N + 8, nh), -7.0, device="cuda")
    sent_lp = torch.full((E.N + 8, 1), -7.0, device="cuda")
    sent_h = torch.full((E.N + 8, 1, 128), -7.0, device="cuda")
    opp._launch(P.AcPolicyRows(E.N, 1, 1, 0, nh), t["obs"], t["rnn_states"], None, t["masks"], False, None, sent_a, sent_lp, sent_h, None,
                COUNTERS[e.derived][-1])
    torch.cuda.current_stream().synchronize()
    assert torch.equal(sent_a[:E.N], out[1]) and torch.equal(sent_lp[:E.N], out[2]) and torch.equal(sent_h[:E.N], out[3])
    assert (sent_a[E.N:] == -7.0).all() and (sent_lp[E.N:] == -7.0).all() and (sent_h[E.N:] == -7.0).all()
    pol.close()
    opp.close()
    problems, used = E.compare(dev, ref, e, E.bounds(e, precision, TOL[e.form]))
    print(f"\n[{name} {precision}] fraction of each bound used: " + "  ".join(f"{k} {v:.3f}" for k, v in used.items()), end="")
    assert problems == [], problems


@pytest.mark.parametrize("precision", ["fast", "fp32"])
@pytest.mark.parametrize("name", ["ppo_d32_8x20_shoot", "wide_129_256"])
def test_pool_members_at_an_edge_configuration(P, name, precision):
    # two members, rows assigned alternately: every row bit-equal to the single policy holding that member's weights
    e, d = E.ENTRIES[name], E.inputs(name)
    o, _, act = spaces(e)
    sds = [d["sd"], E.state_dicts(e._replace(seed=e.seed + 50))[0]]
    pool = P.DevicePolicyPool(o, act, args(e), 2, form=e.form, precision=precision, seed=SEED)
    for k, sd in enumerate(sds):
        pool.load_state_dict(k, sd)
    members = (np.arange(E.N) % 2).astype(np.int32)
    pool.assign(members)
    obs, h, m = cuda(d["obs"]), cuda(d["rnn_states"]), cuda(d["masks"])
    refs = [make(P, e, precision, sd, None) for sd in sds]
    for det, counter in ((True, 0), (False, 9)):
        a, ho, lp = pool.act(obs, h, m, deterministic=det, counter=counter, return_log_probs=True)
        for k, ref in enumerate(refs):
            ar, hr, lr = ref.act(obs, h, m, deterministic=det, counter=counter, return_log_probs=True)
            torch.cuda.current_stream().synchronize()
            sel = torch.as_tensor(members == k).cuda()
            assert torch.equal(a[sel], ar[sel]) and torch.equal(ho[sel], hr[sel]) and torch.equal(lp[sel], lr[sel]), f"member {k} det={det}"
        assert not torch.equal(ho[0::2], refs[1].act(obs, h, m, deterministic=det, counter=counter)[1][0::2])   # the members do differ
    for p in refs + [pool]:
        p.close()
