"""The device PPO policy's host side (no GPU): blob layout, refusals, the keyed generator, and the tests' float64 restatement of the
reference's network pinned to tests/golden/policy_1v1.npz and policy_seeded.npz (which tests/golden/make_policy_golden.py made from the reference's own modules)."""
import importlib
import types

import numpy as np
import pytest

import policy_util as U

pkg = importlib.import_module("aircombat-selfplay_amd")
P = importlib.import_module("aircombat-selfplay_amd.policy")
ve = importlib.import_module("aircombat-selfplay_amd.vec_env")


def _cfg(tag, precision="fast", **kw):
    a = U.args(tag)
    a.__dict__.update(kw)
    obs, act = U.spaces(tag)
    return P.make_config(obs, act, a, precision)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_blob_order_matches_documented_layout(tag):
    g = U.golden()
    asd, csd = U.state_dicts(g, tag)
    cfg = _cfg(tag)
    ka, kc = P.blob_keys(cfg)
    # every tensor of the reference's state_dicts, each once (the checkpoint's keys: base.mlp.fc.{0,2,3,5}, rnn.gru.*_l0, rnn.norm,
    # act.mlp.fc.{0,2,3,5}, act.action_outs.{0..}) -- in state_dict order
    assert ka == list(asd.keys())
    if csd is not None:
        assert kc == list(csd.keys())
    na, nc = P.check_config(cfg)
    blob = P.blob_from_state_dict(cfg, asd)
    assert blob.size == na == sum(v.size for v in asd.values())
    assert np.array_equal(blob, np.concatenate([asd[k].ravel() for k in ka]))
    if csd is not None:
        assert P.blob_from_state_dict(cfg, csd, critic=True).size == nc == sum(v.size for v in csd.values())
    # the documented start of the actor blob: feature norm (when on), then base.mlp.fc.0.weight [128, obs_dim]
    off = 2 * U.CASES[tag][0] if U.CASES[tag][3] else 0
    assert np.array_equal(blob[off:off + 128 * U.CASES[tag][0]], asd["base.mlp.fc.0.weight"].ravel())
    assert np.array_equal(blob[-asd[ka[-1]].size:], asd[ka[-1]].ravel())


REFUSALS = [
    ("activation_id", dict(activation_id=0), "activation_id"),
    ("hidden", dict(hidden_size="64 64"), "hidden sizes"),
    ("act_hidden", dict(act_hidden_size="128"), "hidden sizes"),
    ("recurrent_size", dict(recurrent_hidden_size=64), "recurrent_hidden_size"),
    ("recurrent_layers", dict(recurrent_hidden_layers=2), "recurrent_hidden_layers"),
    ("not_recurrent", dict(use_recurrent_policy=False), "use_recurrent_policy"),
    ("no_prior", dict(use_prior=False), "use_prior"),
]


@pytest.mark.parametrize("name,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_configurations(name, kw, msg):
    with pytest.raises(P.UnsupportedPolicy, match=msg):
        P.check_config(_cfg("a", **kw))


def test_refused_spaces_and_sizes():
    a = U.args("a")
    obs = ve._Box(-10, 10, (21,))
    with pytest.raises(P.UnsupportedPolicy, match="Discrete\\(2\\)"):
        P.check_config(P.make_config(obs, ve._Tuple([ve._MultiDiscrete([3, 5, 3]), ve._Discrete(2)]), a))
    with pytest.raises(P.UnsupportedPolicy, match="Box"):
        P.make_config(obs, ve._Box(-1, 1, (4,)), a)
    MultiBinary = type("MultiBinary", (), {"shape": (4,)})
    with pytest.raises(P.UnsupportedPolicy, match="MultiBinary"):
        P.make_config(obs, MultiBinary(), a)
    with pytest.raises(P.UnsupportedPolicy, match="obs_dim"):
        P.check_config(P.make_config(ve._Box(-10, 10, (33,)), ve._MultiDiscrete([3, 5, 3]), a))
    with pytest.raises(P.UnsupportedPolicy, match="160 logits"):
        P.check_config(P.make_config(obs, ve._MultiDiscrete([41, 41, 41, 41]), a))
    with pytest.raises(P.UnsupportedPolicy, match="obs_dim must be >= 14"):
        P.check_config(P.make_config(ve._Box(-10, 10, (12,)), ve._Tuple([ve._MultiDiscrete([3, 5, 3]), ve._MultiDiscrete([2] * 4)]), a))
    # the supported ones pass, in both forms
    for tag in ("a", "b"):
        for prec in ("fast", "fp32"):
            assert P.check_config(_cfg(tag, prec))[0] > 0


def test_draws_deterministic_and_key_separated():
    base = P.draw_host(11, 5, range(1000, 1100), 2)
    assert np.array_equal(base, P.draw_host(11, 5, range(1000, 1100), 2))
    assert np.array_equal(base[10:20], P.draw_host(11, 5, range(1010, 1020), 2))   # a pure function of the row, not of the batch
    assert base.min() >= 0.0 and base.max() < 1.0
    for other in (P.draw_host(12, 5, range(1000, 1100), 2), P.draw_host(11, 6, range(1000, 1100), 2),
                  P.draw_host(11, 5, range(1000, 1100), 3), P.draw_host(11, 5, range(1001, 1101), 2)):
        assert np.mean(other == base) < 0.02


def test_draws_uniform_chi2():
    u = np.concatenate([P.draw_host(3, c, 250_000, h) for c, h in ((0, 0), (1, 0), (0, 1), (7, 5))])
    assert u.size == 1_000_000
    k = 1000
    counts = np.bincount(np.minimum((u * k).astype(np.int64), k - 1), minlength=k)
    chi2 = ((counts - u.size / k) ** 2 / (u.size / k)).sum()
    # 999 degrees of freedom: mean 999, sd 44.7; 1150 is 3.4 sd out
    assert chi2 < 1150, chi2
    assert abs(u.mean() - 0.5) < 5e-3


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_reproduces_reference_golden(tag):
    # float64 outputs of the fixture to 1e-9; the float32-stored ones (GRU states, logits) to their own rounding (one float32 ulp).
    # The log-probs and values depend on every layer, the GRU included, so the 1e-9 pins the whole restatement.
    g = U.golden()
    asd, csd = U.state_dicts(g, tag)
    obs_dim, nvec, n_shoot, fn, _, has_c = U.CASES[tag]
    out = U.actor(asd, g[f"{tag}_obs"], g[f"{tag}_rnn_states"], g[f"{tag}_masks"], nvec, n_shoot, fn)
    exact64 = ("actions", "log_probs") + (("shoot_p",) if n_shoot else ())
    got = dict(out)
    if has_c:
        got.update(U.critic(csd, g[f"{tag}_obs"], g[f"{tag}_rnn_states_critic"], g[f"{tag}_masks"], fn))
        exact64 += ("values",)
    for k in exact64:
        np.testing.assert_allclose(got[k], g[f"{tag}_{k}"], rtol=0, atol=1e-9, err_msg=k)
    for k in ("rnn_states_out", "logits") + (("rnn_states_critic_out",) if has_c else ()):
        assert g[f"{tag}_{k}"].dtype == np.float32
        np.testing.assert_allclose(got[k], g[f"{tag}_{k}"], rtol=2.0 ** -23, atol=1e-30, err_msg=k)
    assert np.abs(g[f"{tag}_log_probs"]).min() > 0 and len(g[f"{tag}_obs"]) == 256
