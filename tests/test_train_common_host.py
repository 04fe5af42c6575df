"""What the training layers share (aircombat-selfplay_amd/train_common.py), without a GPU: the one walker behind the four use_device_*
functions keeps their promises for each of them, and the launch helper turns the library's refusal of a workspace into its message."""
import ctypes as C
import importlib

import pytest

torch = pytest.importorskip("torch")
nn = torch.nn

import act_train_util as AU   # noqa: E402
import gru_layer_util as GL   # noqa: E402
import mlp_train_util as MU   # noqa: E402


def _mod(name):
    return importlib.import_module("aircombat-selfplay_amd." + name)


# (module, function, an acceptable layer, an unacceptable one, is this object the device form)
CASES = {
    "use_device_gru": ("gru_train", GL.RefGRULayer, lambda: GL.RefGRULayer(layers=2), lambda m: type(m) is _mod("gru_train").DeviceGRULayer),
    "use_device_gru_layer": ("gru_layer_train", GL.RefGRULayer, lambda: GL.RefGRULayer(layers=2),
                             lambda m: type(m) is _mod("gru_layer_train").DeviceFusedGRULayer),
    "use_device_mlp": ("mlp_train", lambda: MU.MLP(12), lambda: MU.MLP(12, act=nn.Tanh()), lambda m: type(m) is _mod("mlp_train").DeviceMLPLayer),
    "use_device_act": ("act_train", lambda: AU.Act((3, 5), ns=1), lambda: AU.Act((3, 5), in_features=64),
                       lambda m: "evaluate_actions" in m.__dict__),
}


@pytest.fixture(params=list(CASES))
def case(request, pkg, monkeypatch):
    name = request.param
    module, good, bad, swapped = CASES[name]
    # a GRU's parameters must be on a CUDA device when it is swapped: with that check lifted (as test_gru_train_host.py and
    # test_gru_layer_host.py lift it) the walk is visible on the CPU, and the layer count is what refuses the bad layer
    monkeypatch.setattr(_mod("gru_train"), "check_gru", lambda gru, where="gru": None)
    monkeypatch.setattr(_mod("gru_layer_train"), "check_layer", lambda gru, norm, where="rnn": None)
    return getattr(_mod(module), name), good, bad, swapped


def _tree(a, b):
    tree = nn.Module()
    tree.a, tree.inner = a, nn.Module()
    tree.inner.b = b
    return tree


def test_one_unacceptable_layer_leaves_every_layer_as_it_was(case, pkg):
    use, good, bad, swapped = case
    tree = _tree(good(), bad())                 # the acceptable one is found first and has passed its check when the other is refused
    a, b = tree.a, tree.inner.b
    with pytest.raises(pkg.UnsupportedPolicy, match=r"inner\.b"):
        use(tree)
    assert tree.a is a and tree.inner.b is b and not swapped(a) and not swapped(b)
    policy = type("PPOPolicy", (), {})()        # the same through an object with actor / critic modules
    policy.actor, policy.critic = _tree(good(), good()), _tree(good(), bad())
    with pytest.raises(pkg.UnsupportedPolicy, match=r"critic\.inner\.b"):
        use(policy)
    assert not any(swapped(m) for root in (policy.actor, policy.critic) for m in root.modules())


def test_second_call_finds_nothing_and_parameters_are_the_same_objects(case):
    use, good, _, swapped = case
    policy = type("PPOPolicy", (), {})()
    policy.actor, policy.critic = _tree(good(), good()), _tree(good(), good())
    roots = (policy.actor, policy.critic)
    params = [p for root in roots for p in root.parameters()]
    keys = [list(root.state_dict()) for root in roots]
    assert use(policy) == 4
    assert all(swapped(root.a) and swapped(root.inner.b) for root in roots)
    assert use(policy) == 0 and use(policy.actor) == 0
    after = [p for root in roots for p in root.parameters()]
    assert len(after) == len(params) and all(p is q for p, q in zip(after, params))
    assert [list(root.state_dict()) for root in roots] == keys


def _act_heads():
    heads = _mod("capi").AcActHeads(n_cat=2, n_shoot_cols=0)   # (by module name, as train_common is: a test before this one may have re-imported the package)
    heads.nvec[:2] = [3, 5]
    return C.byref(heads)


REFUSED = {
    "ac_mlp_block_workspace_floats": lambda: (2 ** 31 - 1, 128),
    "ac_act_eval_workspace_floats": lambda: (_act_heads(), 2 ** 31 - 1),
    "ac_gru_layer_workspace_floats": lambda: (2 ** 31 - 1, 1),
    "ac_ppo_loss_workspace_floats": lambda: (2 ** 31 - 1, 1),
}


@pytest.mark.parametrize("symbol", list(REFUSED))
def test_refused_workspace_is_the_librarys_message(pkg, symbol):
    run = _mod("train_common").Launch(torch.zeros(1))
    with pytest.raises(RuntimeError, match=symbol + r" failed: " + symbol + r": .*32-bit"):
        run.workspace(symbol, *REFUSED[symbol]())
