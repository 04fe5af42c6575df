"""The one-call networks without a GPU (aircombat-selfplay_amd/net_train.py): what use_device_networks refuses, one fault at a time
and with the module path in the message, that nothing is changed after a refusal, the ac_net_t packing and parameter order against a
hand-written table, the two size functions against include/aircombat.h's arithmetic, their refusals, the exports, and deepcopy."""
import copy
import ctypes as C
import importlib

import pytest

import net_train_util as NU

torch = pytest.importorskip("torch")
nn = torch.nn


@pytest.fixture(scope="module")
def Nt(pkg):
    return importlib.import_module("aircombat-selfplay_amd.net_train")


@pytest.fixture(scope="module")
def capi(Nt):
    return Nt.capi   # the very module net_train packs its structs with (the package can be imported under two names)


def _policy(heads="prior", fnorm=True, **kw):
    return NU.Policy(heads, fnorm, device="cpu", **kw)


def _untouched(pol):
    return "evaluate_actions" not in pol.actor.__dict__ and "forward" not in pol.critic.__dict__


def _value_out_two(p): p.critic.value_out = nn.Linear(128, 2)
def _value_out_no_bias(p): p.critic.value_out = nn.Linear(128, 1, bias=False)
def _value_out_narrow(p): p.critic.value_out = nn.Linear(64, 1)
def _fnorm_width(p): p.actor.base.feature_norm = nn.LayerNorm(20)
def _fnorm_no_affine(p): p.critic.base.feature_norm = nn.LayerNorm(21, elementwise_affine=False)
def _not_recurrent(p): p.actor.use_recurrent_policy = False
def _no_rnn(p): del p.critic.rnn
def _tanh(p): p.actor.base.mlp.fc[1] = nn.Tanh()
def _wide_obs(p): p.critic.base.mlp.fc[0] = nn.Linear(300, 128)
def _gru_size(p): p.critic.rnn.gru = nn.GRU(128, 64)
def _rnn_norm(p): p.actor.rnn.norm = nn.LayerNorm(128, elementwise_affine=False)
def _head_in(p): p.actor.act.action_outs[1].logits_net = nn.Linear(64, 5)
def _half(p): p.actor.act.mlp.fc[3].half()
def _no_prior(p): p.actor.use_prior = False


def _five_blocks(p):
    p.critic.mlp = NU.MU.MLP(128, widths=(128,) * 5)


def _single_head(p):
    del p.actor.act.action_outs
    p.actor.act.action_out = nn.Linear(128, 3)


REFUSALS = [(_value_out_two, "critic.value_out", "Linear(128, 2)"), (_value_out_no_bias, "critic.value_out", "without bias"),
            (_value_out_narrow, "critic.value_out", "Linear(64, 1)"), (_fnorm_width, "actor.base.feature_norm", "the input's width is 21"),
            (_fnorm_no_affine, "critic.base.feature_norm", "affine"), (_not_recurrent, "actor.rnn", "use_recurrent_policy=False"),
            (_no_rnn, "critic.rnn", "use_recurrent_policy=False"), (_tanh, "actor.base.mlp.fc.0", "Tanh"),
            (_wide_obs, "critic.base.mlp.fc.0", "in-features 300"), (_gru_size, "critic.rnn.gru", "128 -> 64"),
            (_rnn_norm, "actor.rnn.norm", "affine"), (_head_in, "actor.act.action_outs.1.logits_net", "in-features 64"),
            (_half, "actor.act.mlp.fc.3", "float16"), (_no_prior, "actor.act.action_outs", "use_prior"),
            (_five_blocks, "critic.mlp.fc", "5 blocks"), (_single_head, "actor.act.action_out", "single")]


@pytest.mark.parametrize("break_it, where, what", REFUSALS, ids=[r[0].__name__.strip("_") for r in REFUSALS])
def test_refusals_name_the_module_and_change_nothing(pkg, break_it, where, what):
    pol = _policy()
    break_it(pol)
    with pytest.raises(pkg.UnsupportedPolicy) as exc:
        pkg.use_device_networks(pol)
    assert where + ":" in str(exc.value) and what in str(exc.value), str(exc.value)
    assert _untouched(pol)   # the other network was fine, and still nothing was bound


def test_a_sound_policy_is_bound_after_the_same_faults_are_mended(pkg, Nt):
    pol = _policy()
    assert _untouched(pol)
    ea, fw = pol.actor.evaluate_actions, pol.critic.forward
    keys = (list(pol.actor.state_dict()), list(pol.critic.state_dict()))
    params = [id(p) for g in pol.optimizer.param_groups for p in g["params"]]
    assert pkg.use_device_networks(pol) == 2
    assert pol.actor.__dict__["evaluate_actions"].__func__ is Nt._device_actor_evaluate_actions
    assert pol.critic.__dict__["forward"].__func__ is Nt._device_critic_forward
    assert pol.actor._device_net_original == ea and pol.critic._device_net_original == fw   # the original methods are kept
    assert (list(pol.actor.state_dict()), list(pol.critic.state_dict())) == keys
    assert [id(p) for p in list(pol.actor.parameters()) + list(pol.critic.parameters())] == params
    assert pkg.use_device_networks(pol.critic) == 1 and pol.critic._device_net_original == fw   # again, and on one module
    with pytest.raises(pkg.UnsupportedPolicy, match="neither"):
        pkg.use_device_networks(nn.Linear(3, 3))


@pytest.mark.parametrize("kw", [dict(products="bf16"), dict(dense_products="fp16"), dict(mlp_products=1), dict(products="")])
def test_bad_products_are_value_errors_before_anything_is_looked_at(pkg, kw):
    pol = _policy()
    _value_out_two(pol)   # would be refused, were it looked at
    with pytest.raises(ValueError, match=next(iter(kw))):
        pkg.use_device_networks(pol, **kw)
    assert _untouched(pol)


def test_products_none_keeps_what_a_swapped_layer_carries(pkg):
    pol = _policy()
    pkg.use_device_mlp(pol, products="bf16x3")
    for net, kw in ((pol.actor, dict(products="bf16x3", dense_products="fp32")), (pol.critic, dict(dense_products="bf16x3"))):
        net.rnn = pkg.DeviceFusedGRULayer(gru=net.rnn.gru, norm=net.rnn.norm, **kw)   # (use_device_gru_layer itself wants a CUDA device)
    assert pkg.use_device_networks(pol) == 2
    assert pol.actor._device_net == dict(products="bf16x3", dense_products="fp32", mlp_products="bf16x3")
    assert pol.critic._device_net == dict(products="fp32", dense_products="bf16x3", mlp_products="bf16x3")
    assert pkg.use_device_networks(pol, products="fp32", mlp_products="fp32") == 2
    assert pol.critic._device_net == dict(products="fp32", dense_products="bf16x3", mlp_products="fp32")
    plain = _policy()
    pkg.use_device_networks(plain)
    assert plain.actor._device_net == dict(products="fp32", dense_products="fp32", mlp_products="fp32")
    mixed = _policy()
    pkg.use_device_mlp(mixed.actor.base, products="bf16x3")
    with pytest.raises(pkg.UnsupportedPolicy, match="actor.act.mlp"):
        pkg.use_device_networks(mixed)
    assert _untouched(mixed)


def test_packing_and_parameter_order(pkg, Nt, capi):
    pol = _policy("prior", fnorm=True)
    a, c = pol.actor, pol.critic
    d = Nt.describe(a, "actor.", device=False)
    fc, afc, g = a.base.mlp.fc, a.act.mlp.fc, a.rnn.gru
    table = [a.base.feature_norm.weight, a.base.feature_norm.bias,
             fc[0].weight, fc[0].bias, fc[2].weight, fc[2].bias, fc[3].weight, fc[3].bias, fc[5].weight, fc[5].bias,
             g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0, a.rnn.norm.weight, a.rnn.norm.bias,
             afc[0].weight, afc[0].bias, afc[2].weight, afc[2].bias, afc[3].weight, afc[3].bias, afc[5].weight, afc[5].bias,
             a.act.action_outs[0].logits_net.weight, a.act.action_outs[0].logits_net.bias, a.act.action_outs[1].logits_net.weight,
             a.act.action_outs[1].logits_net.bias, a.act.action_outs[2].logits_net.weight, a.act.action_outs[2].logits_net.bias,
             a.act.action_outs[6].net.weight, a.act.action_outs[6].net.bias]   # of the four shoot heads only the last takes part
    assert [id(p) for p in d.params] == [id(p) for p in table]
    assert (d.kind, d.obs_dim, d.feature_norm, d.base_blocks, d.head_blocks, d.nvec, d.n_shoot) == ("actor", 21, True, 2, 2, (3, 5, 3), 4)
    a.base.feature_norm.eps, fc[5].eps, a.rnn.norm.eps, afc[2].eps = 1e-3, 2e-5, 3e-5, 4e-5
    net = Nt.describe(a, "actor.", device=False).pack("bf16x3", "fp32", "bf16x3")
    assert isinstance(net, capi.AcNet)
    assert (net.obs_dim, net.feature_norm, net.base_blocks, net.head_blocks) == (21, 1, 2, 2)
    assert (net.heads.n_cat, list(net.heads.nvec)[:3], net.heads.n_shoot_cols) == (3, [3, 5, 3], 4)
    assert (net.mlp_products, net.gru_products, net.gru_dense_products) == (1, 0, 1)
    f32 = lambda v: C.c_float(v).value
    assert net.feature_norm_eps == f32(1e-3) and net.gru_eps == f32(3e-5)
    assert list(net.block_eps)[:4] == [f32(1e-5), f32(2e-5), f32(4e-5), f32(1e-5)] and all(p is None for p in net.params)
    dc = Nt.describe(c, "critic.", device=False)
    cfc, mfc = c.base.mlp.fc, c.mlp.fc
    ctable = [c.base.feature_norm.weight, c.base.feature_norm.bias] + [getattr(cfc[j], k) for j in (0, 2, 3, 5) for k in ("weight", "bias")] + \
        [c.rnn.gru.weight_ih_l0, c.rnn.gru.weight_hh_l0, c.rnn.gru.bias_ih_l0, c.rnn.gru.bias_hh_l0, c.rnn.norm.weight, c.rnn.norm.bias] + \
        [getattr(mfc[j], k) for j in (0, 2, 3, 5) for k in ("weight", "bias")] + [c.value_out.weight, c.value_out.bias]
    assert [id(p) for p in dc.params] == [id(p) for p in ctable]
    cnet = dc.pack()
    assert (dc.kind, cnet.heads.n_cat, cnet.heads.n_shoot_cols, cnet.feature_norm) == ("critic", 0, 0, 1)
    plain = Nt.describe(_policy("ppo", fnorm=False).actor, device=False)
    assert len(plain.params) == 8 + 6 + 8 + 8 and not plain.feature_norm and plain.n_shoot == 0 and plain.obs_dim == 15
    assert C.sizeof(capi.AcNet) == 4 * 4 + 40 + 3 * 4 + 4 + 8 * 4 + 4 + 4 + 64 * 8   # include/aircombat.h's ac_net_t, its padding included


def _net(capi, obs_dim=21, fnorm=1, nb=2, nh=2, nvec=(3, 5, 3), ns=4):
    net = capi.AcNet(obs_dim=obs_dim, feature_norm=fnorm, base_blocks=nb, head_blocks=nh)
    net.heads.n_cat, net.heads.n_shoot_cols = len(nvec), ns
    net.heads.nvec[:len(nvec)] = list(nvec)
    return net


@pytest.mark.parametrize("N, T", [(1, 1), (3, 4), (2400, 8)])
def test_sizes_match_their_documented_arithmetic(pkg, capi, N, T):
    lib = capi.load_library()
    for cfg in (dict(), dict(obs_dim=15, fnorm=0, nvec=(41, 41, 41, 30), ns=0), dict(obs_dim=168, nvec=(), ns=0, nb=1, nh=0),
                dict(obs_dim=256, fnorm=0, nvec=(), ns=0, nb=4, nh=4)):
        net = _net(capi, **cfg)
        args = (net.obs_dim, net.feature_norm, net.base_blocks, net.head_blocks, net.heads.n_shoot_cols, N, T)
        assert lib.ac_net_saved_floats(C.byref(net), N, T) == NU.saved_floats(*args), cfg
        heads = net.heads if net.heads.n_cat else None
        assert lib.ac_net_workspace_floats(C.byref(net), N, T) == NU.workspace_floats(lib, heads, *args), cfg
    assert NU.saved_floats(21, 1, 2, 2, 4, 3, 4) == 24 + 252 + 4 * 24 + 5 * 1536 + 1536 + 6144 + 24 + 2 * 12   # one shape by hand


@pytest.mark.parametrize("change, N, said", [(dict(), 0, "N and T"), (dict(obs_dim=257), 4, "obs_dim"), (dict(nb=5), 4, "base_blocks"),
                                            (dict(nh=5), 4, "head_blocks"), (dict(nb=0), 4, "base_blocks"), (dict(obs_dim=13), 4, "14 columns"),
                                            (dict(nvec=(), ns=4), 4, "shoot columns"), (dict(nvec=(3, 1)), 4, "at least 2")])
def test_sizes_refuse_with_a_message(pkg, capi, change, N, said):
    lib = capi.load_library()
    net = _net(capi, **change)
    for fn in (lib.ac_net_workspace_floats, lib.ac_net_saved_floats):
        assert fn(C.byref(net), N, 8) == -1
        assert said in lib.last_error(), lib.last_error()
    bad = _net(capi)
    bad.gru_products = 7
    assert lib.ac_net_saved_floats(C.byref(bad), 4, 8) == -1 and "products" in lib.last_error()
    assert lib.ac_net_saved_floats(None, 4, 8) == -1 and "null" in lib.last_error()
    assert lib.ac_value_head_workspace_floats(0) == -1 and lib.ac_feature_norm_workspace_floats(4, 257) == -1
    assert "1 .. 256" in lib.last_error()


def test_exports(pkg, Nt):
    names = ("DeviceActorEvalFunction", "DeviceCriticFunction", "value_head", "feature_norm", "shoot_prior", "use_device_networks")
    for name in names:
        assert getattr(pkg, name) is getattr(Nt, name) and name in pkg.__all__
    lib = pkg.load_library()
    for symbol in ("ac_net_workspace_floats", "ac_net_saved_floats", "ac_actor_eval_forward", "ac_actor_eval_backward", "ac_critic_forward",
                   "ac_critic_backward", "ac_value_head_forward", "ac_value_head_backward", "ac_feature_norm_forward", "ac_feature_norm_backward",
                   "ac_shoot_prior", "ac_net_constant"):
        assert callable(getattr(lib, symbol))
    assert Nt.constants() == dict(rows=64, forward_workgroups=512, backward_workgroups=256)


def test_deepcopy_runs_the_device_method_on_its_own_parameters(pkg, Nt):
    pol = _policy()
    pkg.use_device_networks(pol, mlp_products="bf16x3")
    twin = copy.deepcopy(pol)
    for net, name, fn in ((twin.actor, "evaluate_actions", Nt._device_actor_evaluate_actions), (twin.critic, "forward", Nt._device_critic_forward)):
        bound = net.__dict__[name]
        assert bound.__func__ is fn and bound.__self__ is net and net._device_net_original.__self__ is net
        assert net._device_net["mlp_products"] == "bf16x3"
    own = {id(p) for p in twin.actor.parameters()}
    assert {id(p) for p in Nt.describe(twin.actor, device=False).params} <= own
    assert not own & {id(p) for p in pol.actor.parameters()}
    # on the CPU the device method is what answers, for the copy's own module: it names the device it cannot run on
    i = NU.inputs(3, 4, 21, (3, 5, 3), 4, device="cpu")
    with pytest.raises(pkg.UnsupportedPolicy, match="only a CUDA device"):
        twin.actor.evaluate_actions(i["obs"], i["rnn_states"], i["action"], i["masks"])
    with pytest.raises(pkg.UnsupportedPolicy, match="only a CUDA device"):
        twin.critic(i["obs"].numpy(), i["rnn_states"].numpy(), i["masks"].numpy())


def test_a_replaced_parameter_or_child_is_noticed(pkg, Nt):
    """What a call re-validates before it trusts the description it read earlier (net_train._Plan.links)."""
    pol = _policy()
    for net in (pol.actor, pol.critic):
        plan = Nt._Plan()
        plan.links = Nt._links(net, Nt.describe(net, device=False).params)
        assert plan.holds() and len(plan.links) > len(list(net.parameters())) // 2
    plan.links = Nt._links(pol.critic, Nt.describe(pol.critic, device=False).params)
    old = pol.critic.value_out
    pol.critic.value_out = nn.Linear(128, 1)            # a child module replaced
    assert not plan.holds()
    pol.critic.value_out = old
    assert plan.holds()
    w = pol.critic.rnn.gru.weight_hh_l0
    pol.critic.rnn.gru.weight_hh_l0 = nn.Parameter(w.detach().clone())   # a Parameter replaced
    assert not plan.holds()
    pol.critic.rnn.gru.weight_hh_l0 = w
    pol.critic.base.mlp.fc[2] = nn.LayerNorm(128)       # a member of an nn.Sequential replaced
    assert not plan.holds()
