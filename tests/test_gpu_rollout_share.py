"""DeviceMAPPORollout.collect (csrc/rollout_collect.hpp) on the MI355X against the stepwise loop it replaces,
built only from the calls that were there before it: get_actions on the buffer's slots (share_obs, obs), the actions written into the
env's action buffer, act_into_env for the opponent, step_device, the share runner's dones_env / zeroing / masks / active_masks and
share_obs in torch, buffer.insert(on_device=True) with the log-probs expanded to act_dim. Both paths run the same kernels on the same
inputs, so everything is compared bit for bit."""
import ctypes as C
import importlib
import types

import numpy as np
import pytest

import policy_util as U

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

E, T = 5, 8            # rows 5 .. 40: no multiple of the policy's 32-row tile or of 64
MAX_STEPS = 5          # every episode times out inside the window; env 1 is crashed before the first step
# case: (task, hierarchical, self-play opponent). "1v1" is the share width that is no multiple of 4 (2 x 15).
CASES = {"mc_all": ("multiplecombat", False, None), "mc_selfplay": ("multiplecombat", False, "policy"),
         "nvn_pool": ("scenario3_nvn", True, "pool"), "1v1": ("singlecombat", False, None)}
FIELDS = ("obs", "share_obs", "actions", "rewards", "masks", "bad_masks", "active_masks", "action_log_probs", "value_preds", "returns",
          "rnn_states_actor", "rnn_states_critic")


@pytest.fixture(scope="module")
def P(pkg):
    return importlib.import_module("aircombat-selfplay_amd.policy")


def args(fn, prior, **kw):
    d = dict(hidden_size="128 128", act_hidden_size="128 128", recurrent_hidden_size=128, recurrent_hidden_layers=1, activation_id=1,
             use_feature_normalization=fn, use_prior=prior, use_recurrent_policy=True, buffer_size=T, n_rollout_threads=E, gamma=0.99,
             gae_lambda=0.95, use_gae=True, use_proper_time_limits=False)
    d.update(kw)
    return types.SimpleNamespace(**d)


def state_dicts(obs_dim, cent_dim, nvec, n_shoot, fn, seed):
    """policy_util's seeded weights as mappo_util builds them: the actor obs_dim wide (plus munition heads when the action space has
    them), the critic cent_dim wide."""
    a = U.seeded_state_dicts(obs_dim, nvec, fn, seed=seed)[0]
    c = U.seeded_state_dicts(cent_dim, nvec, fn, seed=seed)[1]
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
        task, hier, opp_kind = CASES[case]
        cfg = pkg.default_config(task, hierarchical=hier)
        cfg.max_steps = MAX_STEPS
        self.env = env = pkg.HipShareVecEnv(cfg, E, device_id=0, seed=7)
        self.A = A = env.num_agents
        self.D = D = env.obs_dim
        self.na = na = A if opp_kind is None else A // 2
        nvec, n_shoot, _ = P._action_heads(env.action_space)
        self.nh = len(nvec) + n_shoot
        a = args(True, n_shoot > 0)
        cent = env.share_observation_space
        assert cent.shape == (A * D,)
        self.policy = P.DeviceMAPPOPolicy(env.observation_space, cent, env.action_space, a, seed=11)
        self.policy.load_state_dict(*state_dicts(D, A * D, nvec, n_shoot, True, 1201))
        self.policy.counter = 40
        self.buffer = pkg.DeviceSharedReplayBuffer(a, na, env.observation_space, cent, env.action_space)
        self.opp = None
        if opp_kind == "policy":
            self.opp = P.DeviceMAPPOPolicy(env.observation_space, cent, env.action_space, a, seed=12, critic=False)
            self.opp.load_state_dict(state_dicts(D, A * D, nvec, n_shoot, True, 1202)[0])
        elif opp_kind == "pool":
            self.opp = P.DevicePolicyPool(env.observation_space, env.action_space, a, 3, form="mappo", seed=12)
            for k in range(3):
                self.opp.load_state_dict(k, state_dicts(D, A * D, nvec, n_shoot, True, 1210 + k)[0])
            self.opp.assign_split(E, [2, 0, 1], na=A - na)
        if self.opp is not None:
            self.opp.counter = 70
        obs, share = env.reset()
        for ag in range(A):
            env.set_status(1, ag, 1)          # every agent of env 1 crashes: that env is done at the first step, the others are not
        # one learner agent of env 2 is done while its env goes on (active_masks 0 beside masks 1)
        if A > 2:
            env.set_status(2, 0, 1)           # agent 0 crashes; its team mates fly on
        else:
            # With two aircraft a crashed status ends both episodes in the same step: the survivor's SafeReturn sees no enemy alive.
            # The terminations run in agent order and agent 0 reads agent 1's status from before the step, so agent 1 is instead put
            # 1000 m under the altitude limit: it ends by LowAltitude during the first step while agent 0 still sees it alive, and the
            # env ends one step later.
            st = env.get_state(2, 1)
            r = st[:3]                        # position, ft from the Earth's centre: moved along the radius
            drop_ft = (env.get_entity(2, 1)[2] - (cfg.altitude_limit - 1000.0)) / 0.3048
            st[:3] = r * (1.0 - drop_ft / np.linalg.norm(r))
            env.set_state(2, 1, st)
        if fill_slot0:
            self.buffer.set_slot("obs", 0, obs[:, :na])
            self.buffer.set_slot("share_obs", 0, share[:, :na])
        self.reset_obs, self.reset_share = obs, share
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
            self.ro = self.pkg.DeviceMAPPORollout(self.env, self.policy, self.buffer, opponent=self.opp, num_learner_agents=self.na)
        return self.ro

    def stepwise(self, n_steps):
        """INTEGRATION.md §5e's loop with the share runner's insert() in torch, on the buffer's slots."""
        env, pol, buf, na, A, D, nh = self.env, self.policy, self.buffer, self.na, self.A, self.D, self.nh
        act, obs, rew, done, _ = env.device_tensors()
        cur = torch.cuda.current_stream()
        for _ in range(n_steps):
            s = buf.step
            values, actions, logp, ha, hc = pol.get_actions(
                buf.device_tensor("share_obs")[s].reshape(-1, A * D), buf.device_tensor("obs")[s].reshape(-1, D),
                buf.device_tensor("rnn_states_actor")[s].reshape(-1, 1, 128), buf.device_tensor("rnn_states_critic")[s].reshape(-1, 1, 128),
                buf.device_tensor("masks")[s].reshape(-1, 1), counter=pol.counter)
            pol.counter += 1
            act[:, :na, :nh] = actions.view(E, na, nh)
            if self.opp is not None:
                self.opp.act_into_env(env, self.h_opp, self.m_opp, agents=slice(na, A), counter=self.opp.counter)
                self.opp.counter += 1
            env.step_device(stream=cur)
            dones = done.reshape(E, A).bool()
            dones_env = dones.all(dim=1)
            ha, hc = ha.view(E, na, 1, 128), hc.view(E, na, 1, 128)
            ha[dones_env] = 0.0
            hc[dones_env] = 0.0
            masks = torch.ones(E, A, 1, device="cuda")
            masks[dones_env] = 0.0
            active = torch.ones(E, A, 1, device="cuda")
            active[dones] = 0.0
            active[dones_env] = 1.0
            if self.opp is not None:
                self.h_opp.view(E, A - na, 1, 128)[dones_env] = 0.0
                self.m_opp.copy_(masks[:, na:].reshape(-1, 1))
            share = obs.reshape(E, 1, A * D).expand(E, A, A * D)[:, :na]
            ins = [obs[:, :na].contiguous(), share.contiguous(), act[:, :na, :nh].contiguous(), rew[:, :na].contiguous(),
                   masks[:, :na].contiguous(), logp.view(E, na, 1).expand(E, na, nh).contiguous(), values, ha.contiguous(), hc.contiguous()]
            cur.synchronize()                 # insert copies on the buffer's own stream
            buf.insert(*ins, active_masks=active[:, :na].contiguous(), on_device=True)

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


@pytest.mark.parametrize("case", list(CASES))
def test_collect_equals_stepwise_loop(pkg, P, case):
    ref, dev = Side(pkg, P, case), Side(pkg, P, case)
    ref.stepwise(3)
    ref.crash_all()
    ref.stepwise(5)
    want = ref.result(False)
    # the window must show the selective zeroing: a step where some but not all envs are done, and one where all are ...
    masks, active = want["buffer.masks"][1:, :, :, 0], want["buffer.active_masks"][1:, :, :, 0]
    gone = (masks[:, :, 0] == 0.0).sum(axis=1)
    assert ((gone > 0) & (gone < E)).any() and (gone == E).any(), gone
    # ... an agent done while its env goes on (env 2: the crashed agent 0, or with two aircraft agent 1 under the altitude limit) ...
    assert ((active == 0.0) & (masks == 1.0)).any(), (active[:, 2], masks[:, 2])
    assert set(np.unique(active)) <= {0.0, 1.0} and not ((active == 0.0) & (masks == 0.0)).any()
    # ... and live states and values, share_obs rows that are the env's block, log-probs once per head column
    assert np.abs(want["buffer.rnn_states_actor"][1:]).max() > 0 and np.abs(want["buffer.value_preds"][:T]).max() > 0
    so = want["buffer.share_obs"]
    assert np.abs(so).max() > 0 and (so == so[:, :, :1]).all()
    lp = want["buffer.action_log_probs"]
    assert np.abs(lp).max() > 0 and (lp == lp[..., :1]).all()
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
    ref, dev = Side(pkg, P, "mc_selfplay"), Side(pkg, P, "mc_selfplay")
    ro = dev.rollout()
    for k in range(2):
        ref.stepwise(T)
        assert ro.collect() == T
        # compute(): get_values on the last slot's share_obs and compute_returns, by hand on the stepwise side
        b = ref.buffer
        nv = ref.policy.get_values(b.device_tensor("share_obs")[T].reshape(-1, ref.A * ref.D), b.device_tensor("rnn_states_critic")[T],
                                   b.device_tensor("masks")[T])
        torch.cuda.current_stream().synchronize()
        b.compute_returns(nv, on_device=True)
        nv_dev = ro.compute_returns()
        assert torch.equal(nv, nv_dev) and nv.abs().max() > 0
        want, got = ref.result(False), dev.result(True)
        assert_same(got, want)
        assert np.abs(want["buffer.returns"]).max() > 0
        ref.buffer.after_update()
        dev.buffer.after_update()
        assert dev.buffer.step == 0
    ref.close()
    dev.close()


def test_collect_is_ordered_on_the_callers_stream(pkg, P):
    ref = Side(pkg, P, "mc_all")
    ref.rollout().collect()
    want = ref.result(True)
    want_rew = want["buffer.rewards"].copy()
    dev = Side(pkg, P, "mc_all", fill_slot0=False)       # slot 0's obs and share_obs are still zero
    ro = dev.rollout()
    slot0, share0 = dev.buffer.device_tensor("obs")[0], dev.buffer.device_tensor("share_obs")[0]
    rewards = dev.buffer.device_tensor("rewards")
    src = torch.as_tensor(dev.reset_obs[:, :dev.na]).pin_memory()
    src_share = torch.as_tensor(np.ascontiguousarray(dev.reset_share[:, :dev.na])).pin_memory()
    side = torch.cuda.Stream()
    after_sleep = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(100_000_000)                   # tens of milliseconds: everything below is queued long before it ends
        after_sleep.record(side)
        slot0.copy_(src, non_blocking=True)              # what the first step acts on lands after the call is queued
        share0.copy_(src_share, non_blocking=True)
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
    s = Side(pkg, P, "mc_selfplay")
    env, pol, buf, opp = s.env, s.policy, s.buffer, s.opp
    A, D, na = s.A, s.D, s.na
    before = s.result(False)
    MR = pkg.DeviceMAPPORollout
    a = args(True, False)
    o_sp, c_sp, a_sp = env.observation_space, env.share_observation_space, env.action_space
    made = []

    def make(kind, *pos, **kw):
        x = kind(*pos, **kw)
        made.append(x)
        return x

    SB, MP = pkg.DeviceSharedReplayBuffer, P.DeviceMAPPOPolicy
    box = lambda n: ve._Box(-10, 10, (n,))
    nvec = [41, 41, 41, 30]
    sd_a = state_dicts(D, A * D, nvec, 0, True, 1201)[0]
    if torch.cuda.device_count() > 1:                    # handles on different devices
        with pytest.raises(ValueError, match="device differs"):
            MR(env, make(MP, o_sp, c_sp, a_sp, a, device_id=1), buf, opponent=opp)
    with pytest.raises(ValueError, match="PPO-form policy"):
        MR(env, make(P.DevicePolicy, o_sp, a_sp, a), buf, opponent=opp)
    with pytest.raises(ValueError, match="without share_obs"):
        MR(env, pol, make(pkg.DeviceReplayBuffer, a, na, o_sp, a_sp), opponent=opp)
    with pytest.raises(ValueError, match="share_obs_dim differs"):
        MR(env, pol, make(SB, a, na, o_sp, box(A * D + 4), a_sp), opponent=opp)
    with pytest.raises(ValueError, match="cent_obs_dim differs"):
        MR(env, make(MP, o_sp, box(A * D + 4), a_sp, a), buf, opponent=opp)
    # (DeviceSharedReplayBuffer always stores the log-probs act_dim wide: the odd one is built through the C ABI)
    odd = pkg.capi.AcBufferConfig(T, E, na, D, A * D, s.nh, 1, 1, 128, 1, 0, 0.99, 0.95)
    odd_h = env.lib.ac_buffer_create(C.byref(odd), 0)
    assert odd_h
    with pytest.raises(ValueError, match="logp_dim differs"):
        MR(env, pol, types.SimpleNamespace(_h=odd_h), opponent=opp)
    env.lib.ac_buffer_destroy(odd_h)
    with pytest.raises(ValueError, match="E differs"):
        MR(env, pol, make(SB, args(True, False, n_rollout_threads=E + 1), na, o_sp, c_sp, a_sp), opponent=opp)
    with pytest.raises(ValueError, match="na differs"):
        MR(env, pol, make(SB, a, na + 1, o_sp, c_sp, a_sp), opponent=opp)
    with pytest.raises(ValueError, match="obs_dim differs"):
        MR(env, make(MP, box(D + 1), c_sp, a_sp, a), buf, opponent=opp)
    with pytest.raises(ValueError, match="obs_dim differs"):
        MR(env, pol, make(SB, a, na, box(D + 1), c_sp, a_sp), opponent=opp)
    with pytest.raises(ValueError, match="act_dim differs"):
        MR(env, pol, make(SB, a, na, o_sp, c_sp, ve._MultiDiscrete([3, 5, 3])), opponent=opp)
    with pytest.raises(ValueError, match="act_dim differs"):
        MR(env, make(MP, o_sp, c_sp, ve._MultiDiscrete([3, 5, 3, 2, 2]), a), buf, opponent=opp)
    with pytest.raises(ValueError, match="hidden size differs"):
        MR(env, pol, make(SB, args(True, False, recurrent_hidden_size=64), na, o_sp, c_sp, a_sp), opponent=opp)
    with pytest.raises(ValueError, match="no critic"):
        MR(env, opp, buf, opponent=opp)
    with pytest.raises(ValueError, match="na must be A or A / 2"):
        MR(env, pol, buf, opponent=opp, num_learner_agents=1)
    with pytest.raises(ValueError, match=r"opponent_kind 0 \(none\) does not fit"):
        MR(env, pol, buf, opponent=None, num_learner_agents=na)
    with pytest.raises(ValueError, match="does not fit A - na = 0"):
        MR(env, pol, make(SB, a, A, o_sp, c_sp, a_sp), opponent=opp, num_learner_agents=A)
    ppo_opp = make(P.DevicePolicy, o_sp, a_sp, a, critic=False)
    with pytest.raises(ValueError, match="PPO-form opponent policy"):
        MR(env, pol, buf, opponent=ppo_opp)
    ppo_pool = make(P.DevicePolicyPool, o_sp, a_sp, a, 2)
    ppo_pool.load_state_dict(0, sd_a)
    ppo_pool.assign(np.zeros(E, np.int32), na=A - na)
    with pytest.raises(ValueError, match="PPO-form opponent pool"):
        MR(env, pol, buf, opponent=ppo_pool)
    pool = make(P.DevicePolicyPool, o_sp, a_sp, a, 2, form="mappo")
    pool.load_state_dict(0, sd_a)
    with pytest.raises(ValueError, match="no assignment"):
        MR(env, pol, buf, opponent=pool)
    pool.assign(np.zeros(E + 2, np.int32), na=A - na)
    with pytest.raises(ValueError, match="E differs"):
        MR(env, pol, buf, opponent=pool)
    with pytest.raises(TypeError, match="opponent is None"):
        MR(env, pol, buf, opponent=object())
    # collect's own refusals
    ro = s.rollout()
    for n in (0, -2):
        with pytest.raises(ValueError, match="n_steps must be at least 1"):
            ro.collect(n)
    with pytest.raises(ValueError, match="runs past buffer_size"):
        ro.collect(T + 1)
    unloaded = make(MP, o_sp, c_sp, a_sp, a)
    ro_unloaded = make(MR, env, unloaded, buf, opponent=opp)
    with pytest.raises(ValueError, match="learner's weights are not loaded"):
        ro_unloaded.collect(1)
    unloaded_opp = make(MP, o_sp, c_sp, a_sp, a, critic=False)
    ro_unloaded_opp = make(MR, env, pol, buf, opponent=unloaded_opp)
    with pytest.raises(ValueError, match="opponent's weights are not loaded"):
        ro_unloaded_opp.collect(1)
    assert unloaded.counter == 0 and unloaded_opp.counter == 0
    assert_same(s.result(False), before)                 # nothing moved: buffer, env, counters
    # a hierarchical env whose controller was never loaded (HipVecEnv always loads it: the handle is made through the C ABI)
    hcfg = pkg.default_config("hierarchical_multiplecombat")
    hh = C.c_void_p()
    env.lib.check(env.lib.ac_create(C.byref(hcfg), E, 0, 7, C.byref(hh)), "ac_create")
    hD, hA = env.lib.ac_obs_dim(hh), int(hcfg.n_agents)
    bare = types.SimpleNamespace(lib=env.lib, _h=hh, num_agents=hA, num_envs=E)
    h_act = ve._MultiDiscrete([3, 5, 3])
    hpol = make(MP, box(hD), box(hA * hD), h_act, a)
    hpol.load_state_dict(*state_dicts(hD, hA * hD, [3, 5, 3], 0, True, 1203))
    hbuf = make(SB, a, hA, box(hD), box(hA * hD), h_act)
    hro = make(MR, bare, hpol, hbuf)
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
