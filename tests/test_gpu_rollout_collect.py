"""DeviceRollout.collect (csrc/rollout_collect.hpp) on the MI355X against the stepwise loop it replaces, built only from the calls that
were there before it: get_actions on the buffer's slot, the actions written into the env's action buffer, act_into_env for the opponent,
step_device, the runners' dones_env / zeroing / masks in torch, buffer.insert(on_device=True). Both paths run the same kernels on the
same inputs, so everything is compared bit for bit."""
import ctypes as C
import importlib
import types

import numpy as np
import pytest

import policy_util as U

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

E, T = 5, 8            # rows 5 / 10: no multiple of the policy's 32-row tile or of 64
MAX_STEPS = 5          # every episode times out inside the window; env 1 is crashed before the first step
CASES = ["1v1", "selfplay_policy", "pool_2v2", "hierarchical"]
FIELDS = ("obs", "actions", "rewards", "masks", "bad_masks", "action_log_probs", "value_preds", "returns", "rnn_states_actor", "rnn_states_critic")


@pytest.fixture(scope="module")
def P(pkg):
    return importlib.import_module("aircombat-selfplay_amd.policy")


def args(fn, prior):
    return types.SimpleNamespace(hidden_size="128 128", act_hidden_size="128 128", recurrent_hidden_size=128, recurrent_hidden_layers=1,
                                 activation_id=1, use_feature_normalization=fn, use_prior=prior, use_recurrent_policy=True,
                                 buffer_size=T, n_rollout_threads=E, gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False)


def state_dicts(obs_dim, nvec, n_shoot, fn, seed):
    """policy_util's seeded actor and critic, plus munition heads when the action space has them."""
    a, c = U.seeded_state_dicts(obs_dim, nvec, fn, seed=seed)
    b = np.float32(1.0 / np.sqrt(128))
    for s in range(n_shoot):
        k = len(nvec) + s
        a[f"act.action_outs.{k}.net.weight"] = (U.hashed(seed * 1000 + 300 + s, 256) * b).reshape(2, 128)
        a[f"act.action_outs.{k}.net.bias"] = U.hashed(seed * 1000 + 400 + s, 2) * b
    return a, c


class Side:
    """One set of handles for a case: env, learner, buffer, opponent. Two Sides of a case are built alike."""

    def __init__(self, pkg, P, case, fill_slot0=True):
        self.pkg, self.case = pkg, case
        task, hier = {"1v1": ("singlecombat", False), "selfplay_policy": ("singlecombat", False), "pool_2v2": ("multiplecombat", False),
                      "hierarchical": ("scenario1", True)}[case]
        cfg = pkg.default_config(task, hierarchical=hier)
        cfg.max_steps = MAX_STEPS
        self.env = env = pkg.HipVecEnv(cfg, E, device_id=0, seed=7)
        self.A = A = env.num_agents
        self.na = na = A if case in ("1v1", "hierarchical") else A // 2
        nvec, n_shoot, _ = P._action_heads(env.action_space)
        self.nh = len(nvec) + n_shoot
        a = args(True, n_shoot > 0)
        self.policy = P.DevicePolicy(env.observation_space, env.action_space, a, seed=11)
        self.policy.load_state_dict(*state_dicts(env.obs_dim, nvec, n_shoot, True, 1201))
        self.policy.counter = 40
        self.buffer = pkg.DeviceReplayBuffer(a, na, env.observation_space, env.action_space)
        self.opp = None
        if case == "selfplay_policy":
            self.opp = P.DevicePolicy(env.observation_space, env.action_space, a, seed=12, critic=False)
            self.opp.load_state_dict(state_dicts(env.obs_dim, nvec, n_shoot, True, 1202)[0])
        elif case == "pool_2v2":
            self.opp = P.DevicePolicyPool(env.observation_space, env.action_space, a, 3, seed=12)
            for k in range(3):
                self.opp.load_state_dict(k, state_dicts(env.obs_dim, nvec, n_shoot, True, 1210 + k)[0])
            self.opp.assign_split(E, [2, 0, 1], na=A - na)
        if self.opp is not None:
            self.opp.counter = 70
        obs = env.reset()
        for ag in range(A):
            env.set_status(1, ag, 1)          # every agent of env 1 crashes: that env is done at the first step, the others are not
        if fill_slot0:
            self.buffer.set_slot("obs", 0, obs[:, :na])
        self.reset_obs = obs
        self.ro = None
        # the stepwise path's opponent bookkeeping (the collector owns its own)
        self.h_opp = torch.zeros(E * (A - na), 1, 128, device="cuda")
        self.m_opp = torch.ones(E * (A - na), 1, device="cuda")

    def crash_all(self):
        """Every agent of every env crashes: the next step ends all episodes at once (a timeout alone never does: env 1, restarted at
        the first step, runs one step behind the others)."""
        for e in range(E):
            for ag in range(self.A):
                self.env.set_status(e, ag, 1)

    def rollout(self):
        if self.ro is None:
            self.ro = self.pkg.DeviceRollout(self.env, self.policy, self.buffer, opponent=self.opp, num_learner_agents=self.na)
        return self.ro

    def stepwise(self, n_steps):
        """INTEGRATION.md §5d's loop with the runners' insert() in torch, on the buffer's slots."""
        env, pol, buf, na, A, nh = self.env, self.policy, self.buffer, self.na, self.A, self.nh
        act, obs, rew, done, _ = env.device_tensors()
        cur = torch.cuda.current_stream()
        for _ in range(n_steps):
            s = buf.step
            values, actions, logp, ha, hc = pol.get_actions(
                buf.device_tensor("obs")[s].reshape(-1, env.obs_dim), buf.device_tensor("rnn_states_actor")[s].reshape(-1, 1, 128),
                buf.device_tensor("rnn_states_critic")[s].reshape(-1, 1, 128), buf.device_tensor("masks")[s].reshape(-1, 1), counter=pol.counter)
            pol.counter += 1
            act[:, :na, :nh] = actions.view(E, na, nh)
            if self.opp is not None:
                self.opp.act_into_env(env, self.h_opp, self.m_opp, agents=slice(na, A), counter=self.opp.counter)
                self.opp.counter += 1
            env.step_device(stream=cur)
            dones_env = done.reshape(E, A).bool().all(dim=1)
            ha, hc = ha.view(E, na, 1, 128), hc.view(E, na, 1, 128)
            ha[dones_env] = 0.0
            hc[dones_env] = 0.0
            masks = torch.ones(E, A, 1, device="cuda")
            masks[dones_env] = 0.0
            if self.opp is not None:
                self.h_opp.view(E, A - na, 1, 128)[dones_env] = 0.0
                self.m_opp.copy_(masks[:, na:].reshape(-1, 1))
            ins = [obs[:, :na].contiguous(), act[:, :na, :nh].contiguous(), rew[:, :na].contiguous(), masks[:, :na].contiguous(), logp, values,
                   ha.contiguous(), hc.contiguous()]
            cur.synchronize()                 # insert copies on the buffer's own stream
            buf.insert(*ins, on_device=True)

    def result(self, collected):
        torch.cuda.synchronize()
        self.env.sync()
        out = {f"buffer.{k}": self.buffer.array(k) for k in FIELDS}
        out["buffer.step"] = np.array(self.buffer.step)
        out["checksum"] = np.array(self.env.full_state_checksum(), dtype=np.uint64)
        for name, t in zip(("act", "obs", "rew", "done", "info"), self.env.device_tensors()):
            out["env." + name] = t.cpu().numpy()
        out["counter"] = np.array(self.policy.counter)
        if self.opp is not None:
            out["opp.counter"] = np.array(self.opp.counter)
            out["opp.h"] = (self.ro.opponent_states if collected else self.h_opp).cpu().numpy()
            out["opp.masks"] = (self.ro.opponent_masks if collected else self.m_opp).cpu().numpy()
        return out

    def close(self):
        for x in (self.ro, self.opp, self.policy, self.buffer, self.env):
            if x is not None:
                x.close()


def bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def assert_same(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), k


@pytest.mark.parametrize("case", CASES)
def test_collect_equals_stepwise_loop(pkg, P, case):
    ref, dev = Side(pkg, P, case), Side(pkg, P, case)
    ref.stepwise(3)
    ref.crash_all()
    ref.stepwise(5)
    want = ref.result(False)
    # the window must show the selective zeroing: a step where some but not all envs are done, and one where all are
    gone = (want["buffer.masks"][1:, :, 0, 0] == 0.0).sum(axis=1)
    assert ((gone > 0) & (gone < E)).any() and (gone == E).any(), gone
    assert np.abs(want["buffer.rnn_states_actor"][1:]).max() > 0 and np.abs(want["buffer.value_preds"][:T]).max() > 0
    ro = dev.rollout()
    assert ro.collect(3) == 3 and dev.buffer.step == 3
    dev.crash_all()
    assert ro.collect(5) == 5
    assert_same(dev.result(True), want)
    if ref.opp is not None:
        assert np.abs(want["opp.h"]).max() > 0
    ref.close()
    dev.close()


def test_second_rollout_after_update(pkg, P):
    ref, dev = Side(pkg, P, "selfplay_policy"), Side(pkg, P, "selfplay_policy")
    ro = dev.rollout()
    for k in range(2):
        ref.stepwise(T)
        assert ro.collect() == T
        # compute(): get_values on the last slot and compute_returns, by hand on the stepwise side
        b = ref.buffer
        nv = ref.policy.get_values(b.device_tensor("obs")[T].reshape(-1, ref.env.obs_dim), b.device_tensor("rnn_states_critic")[T],
                                   b.device_tensor("masks")[T])
        torch.cuda.current_stream().synchronize()
        b.compute_returns(nv, on_device=True)
        nv_dev = ro.compute_returns()
        assert torch.equal(nv, nv_dev)
        want, got = ref.result(False), dev.result(True)
        assert_same(got, want)
        assert np.abs(want["buffer.returns"]).max() > 0
        ref.buffer.after_update()
        dev.buffer.after_update()
        assert dev.buffer.step == 0
    ref.close()
    dev.close()


def test_collect_is_ordered_on_the_callers_stream(pkg, P):
    ref = Side(pkg, P, "1v1")
    ref.rollout().collect()
    want = ref.result(True)
    want_rew = want["buffer.rewards"].copy()
    dev = Side(pkg, P, "1v1", fill_slot0=False)          # slot 0's obs is still zero
    ro = dev.rollout()
    slot0 = dev.buffer.device_tensor("obs")[0]
    rewards = dev.buffer.device_tensor("rewards")
    src = torch.as_tensor(dev.reset_obs[:, :dev.na]).pin_memory()
    side = torch.cuda.Stream()
    after_sleep = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(100_000_000)                   # tens of milliseconds: everything below is queued long before it ends
        after_sleep.record(side)
        slot0.copy_(src, non_blocking=True)              # the observations the first step acts on land after the call is queued
        ro.collect()
        returned_early = not after_sleep.query()
        rew = rewards.clone()                            # a torch reader on the same stream
    assert returned_early, "collect waited for the work queued ahead of it"
    side.synchronize()
    assert np.array_equal(bits(rew.cpu().numpy()), bits(want_rew))
    assert_same(dev.result(True), want)
    ref.close()
    dev.close()


def test_refusals(pkg, P):
    """One case per refusal. The "handles on different devices" case needs a second GPU: where the machine shows one device it cannot
    be built and is the only refusal left without a test."""
    ve = importlib.import_module("aircombat-selfplay_amd.vec_env")
    s = Side(pkg, P, "selfplay_policy")
    env, pol, buf, opp = s.env, s.policy, s.buffer, s.opp
    before = s.result(False)
    DR = pkg.DeviceRollout
    a = args(True, False)
    made = []

    def make(kind, **kw):
        x = kind(**kw) if not isinstance(kind, tuple) else kind[0](*kind[1], **kw)
        made.append(x)
        return x

    nvec = [41, 41, 41, 30]
    sd_a, sd_c = state_dicts(env.obs_dim, nvec, 0, True, 1201)
    if torch.cuda.device_count() > 1:                    # handles on different devices
        other = make((P.DevicePolicy, (env.observation_space, env.action_space, a)), device_id=1)
        with pytest.raises(ValueError, match="device differs"):
            DR(env, other, buf, opponent=opp)
    with pytest.raises(ValueError, match="E differs"):
        DR(env, pol, make((pkg.DeviceReplayBuffer, (types.SimpleNamespace(**{**vars(a), "n_rollout_threads": E + 1}), 1, env.observation_space,
                                                    env.action_space))), opponent=opp)
    with pytest.raises(ValueError, match="na differs"):
        DR(env, pol, make((pkg.DeviceReplayBuffer, (a, 2, env.observation_space, env.action_space))), opponent=opp)
    with pytest.raises(ValueError, match="obs_dim differs"):
        DR(env, make((P.DevicePolicy, (ve._Box(-10, 10, (env.obs_dim + 1,)), env.action_space, a))), buf, opponent=opp)
    with pytest.raises(ValueError, match="obs_dim differs"):
        DR(env, pol, make((pkg.DeviceReplayBuffer, (a, 1, ve._Box(-10, 10, (env.obs_dim + 1,)), env.action_space))), opponent=opp)
    with pytest.raises(ValueError, match="act_dim differs"):
        DR(env, pol, make((pkg.DeviceReplayBuffer, (a, 1, env.observation_space, ve._MultiDiscrete([3, 5, 3])))), opponent=opp)
    with pytest.raises(ValueError, match="act_dim differs"):
        DR(env, make((P.DevicePolicy, (env.observation_space, ve._MultiDiscrete([3, 5, 3, 2, 2]), a))), buf, opponent=opp)
    with pytest.raises(ValueError, match="hidden size differs"):
        DR(env, pol, make((pkg.DeviceReplayBuffer, (types.SimpleNamespace(**{**vars(a), "recurrent_hidden_size": 64}), 1, env.observation_space,
                                                    env.action_space))), opponent=opp)
    cent = ve._Box(-10, 10, (env.num_agents * env.obs_dim,))
    with pytest.raises(ValueError, match="MAPPO-form policy"):
        DR(env, make((P.DeviceMAPPOPolicy, (env.observation_space, cent, env.action_space, a))), buf, opponent=opp)
    with pytest.raises(ValueError, match="shared buffer"):
        DR(env, pol, make((pkg.DeviceSharedReplayBuffer, (a, 1, env.observation_space, cent, env.action_space))), opponent=opp)
    with pytest.raises(ValueError, match="no critic"):
        DR(env, opp, buf, opponent=opp)
    env4 = make((pkg.HipVecEnv, (pkg.default_config("multiplecombat"), E)))
    with pytest.raises(ValueError, match="na must be A or A / 2"):
        DR(env4, pol, buf, opponent=opp, num_learner_agents=1)
    with pytest.raises(ValueError, match=r"opponent_kind 0 \(none\) does not fit"):
        DR(env, pol, buf, opponent=None, num_learner_agents=1)
    with pytest.raises(ValueError, match="does not fit A - na = 0"):
        DR(env, pol, make((pkg.DeviceReplayBuffer, (a, 2, env.observation_space, env.action_space))), opponent=opp, num_learner_agents=2)
    pool = make((P.DevicePolicyPool, (env.observation_space, env.action_space, a, 2)))
    pool.load_state_dict(0, sd_a)
    with pytest.raises(ValueError, match="no assignment"):
        DR(env, pol, buf, opponent=pool)
    pool.assign(np.zeros(E + 2, np.int32), na=1)
    with pytest.raises(ValueError, match="E differs"):
        DR(env, pol, buf, opponent=pool)
    wide = make((P.DevicePolicyPool, (env.observation_space, env.action_space, a, 2)), form="mappo")
    wide.load_state_dict(0, sd_a)
    wide.assign(np.zeros(E, np.int32), na=1)
    with pytest.raises(ValueError, match="MAPPO-form opponent pool"):
        DR(env, pol, buf, opponent=wide)
    # collect's own refusals
    ro = s.rollout()
    for n in (0, -2):
        with pytest.raises(ValueError, match="n_steps must be at least 1"):
            ro.collect(n)
    with pytest.raises(ValueError, match="runs past buffer_size"):
        ro.collect(T + 1)
    # weights that were never loaded: refused by the loop the two rollout forms and the evaluator share, before anything is queued
    unloaded = make((P.DevicePolicy, (env.observation_space, env.action_space, a)))
    ro_unloaded = make((DR, (env, unloaded, buf)), opponent=opp)
    with pytest.raises(ValueError, match="learner's weights are not loaded"):
        ro_unloaded.collect(1)
    assert buf.step == 0 and unloaded.counter == 0 and opp.counter == 70
    unloaded_opp = make((P.DevicePolicy, (env.observation_space, env.action_space, a)), critic=False)
    ro_unloaded_opp = make((DR, (env, pol, buf)), opponent=unloaded_opp)
    with pytest.raises(ValueError, match="opponent's weights are not loaded"):
        ro_unloaded_opp.collect(1)
    assert buf.step == 0 and pol.counter == 40 and unloaded_opp.counter == 0
    assert_same(s.result(False), before)                 # nothing moved: buffer, env, counters
    # a hierarchical env whose controller was never loaded (HipVecEnv always loads it: the handle is made through the C ABI)
    hcfg = pkg.default_config("hierarchical_multiplecombat")
    hh = C.c_void_p()
    env.lib.check(env.lib.ac_create(C.byref(hcfg), E, 0, 7, C.byref(hh)), "ac_create")
    hD, hA = env.lib.ac_obs_dim(hh), int(hcfg.n_agents)
    bare = types.SimpleNamespace(lib=env.lib, _h=hh, num_agents=hA, num_envs=E)
    h_obs, h_act = ve._Box(-10, 10, (hD,)), ve._MultiDiscrete([3, 5, 3])
    hpol = make((P.DevicePolicy, (h_obs, h_act, a)))
    hpol.load_state_dict(*state_dicts(hD, [3, 5, 3], 0, True, 1203))
    hbuf = make((pkg.DeviceReplayBuffer, (a, hA, h_obs, h_act)))
    hro = make((DR, (bare, hpol, hbuf)))
    hbefore = {k: hbuf.array(k) for k in FIELDS}
    with pytest.raises(ValueError, match="ac_load_controller has not been called"):
        hro.collect(1)
    torch.cuda.synchronize()
    assert hbuf.step == 0 and hpol.counter == 0
    for k in FIELDS:
        assert np.array_equal(bits(hbuf.array(k)), bits(hbefore[k])), k
    hro.close()
    env.lib.ac_destroy(hh)
    ro.collect(T - 2)
    mid = s.result(False)
    with pytest.raises(ValueError, match="runs past buffer_size"):
        ro.collect(3)
    assert_same(s.result(False), mid)
    assert s.buffer.step == T - 2 and s.policy.counter == 40 + T - 2 and s.opp.counter == 70 + T - 2
    for x in reversed(made):
        x.close()
    s.close()
