"""DeviceLeague (csrc/league_collect.hpp) and the pool's sided plan (csrc/policy_pool.hpp) on the MI355X: the sided launch against
single policies holding each side's member, run(n) against the stepwise loop of the same launches with the bookkeeping in torch, the
payoff table against its host twin and against the numpy restatement, and the refusals that need a device. Both sides of every
comparison run the same arithmetic, so everything is compared bit for bit."""
import ctypes as C
import importlib
import types

import numpy as np
import pytest

import policy_util as U
from league_util import TIMEOUT, assert_table, table_loop, threshold_log

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K, CAP = 2, 3
MAX_STEPS = 5          # every episode times out inside a few steps; env 1 is crashed before the first step, so it runs out of phase
# case: (task, MAPPO-form members, E): 56 envs of 1v1 are 112 half-env rows over 3 members, so each member's rows cross the 32-row tile
CASES = {"1v1": ("singlecombat", False, 56), "2v2": ("multiplecombat", False, 20), "2v2_mappo": ("multiplecombat", True, 20)}


@pytest.fixture(scope="module")
def P(pkg):
    return importlib.import_module("aircombat-selfplay_amd.policy")


def args(prior):
    return types.SimpleNamespace(hidden_size="128 128", act_hidden_size="128 128", recurrent_hidden_size=128, recurrent_hidden_layers=1,
                                 activation_id=1, use_feature_normalization=True, use_prior=prior, use_recurrent_policy=True)


class Side:
    """One set of handles for a case: env, a pool of CAP loaded members under round_robin's sided assignment, and the stepwise path's
    own state in torch. Two Sides of a case are built alike."""

    def __init__(self, pkg, P, case, capacity=CAP, pair=True, E=None):
        self.pkg, self.P, self.case = pkg, P, case
        task, self.mappo, self.E = CASES[case]
        self.E = E or self.E
        cfg = pkg.default_config(task)
        cfg.max_steps = MAX_STEPS
        self.env = env = (pkg.HipShareVecEnv if self.mappo else pkg.HipVecEnv)(cfg, self.E, device_id=0, seed=7)
        self.A = env.num_agents
        self.nvec, self.n_shoot, _ = P._action_heads(env.action_space)
        self.nh = len(self.nvec) + self.n_shoot
        self.args = args(self.n_shoot > 0)
        self.sds = [U.add_munition_heads(U.seeded_state_dicts(env.obs_dim, self.nvec, True, seed=1300 + k)[0], len(self.nvec), self.n_shoot, 1300 + k)
                    for k in range(CAP)]
        self.pool = P.DevicePolicyPool(env.observation_space, env.action_space, self.args, capacity, form="mappo" if self.mappo else "ppo", seed=12)
        for k, sd in enumerate(self.sds):
            self.pool.load_state_dict(k, sd)
        self.pool.counter = 70
        self.members2 = pkg.round_robin(self.E, range(CAP))
        if pair:
            self.pool.assign_sides(self.members2, self.A)
        self.lg = None
        self.reset()

    def reset(self):
        self.env.reset()
        for ag in range(self.A):
            self.env.set_status(1, ag, 1)          # every agent of env 1 crashes: that env is done at the first step, the others are not
        E, A = self.E, self.A
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
        self.h, self.m = z(E * A, 1, 128), torch.ones(E * A, 1, device="cuda")
        self.cum, self.len, self.count = z(E, A), z(E, dt=torch.int32), z(E, dt=torch.int32)
        self.log_ret = z(E, K, A)
        self.log_len, self.log_end, self.log_code = (z(E, K, dt=torch.int32) for _ in range(3))
        self.remaining, self.t = E, 0

    def single(self, member):
        """an actor-only policy of the pool's form holding member ``member``, with the pool's seed"""
        P, env = self.P, self.env
        if self.mappo:
            cent = importlib.import_module("aircombat-selfplay_amd.vec_env")._Box(-10, 10, (self.A * env.obs_dim,))
            p = P.DeviceMAPPOPolicy(env.observation_space, cent, env.action_space, self.args, seed=12, critic=False)
        else:
            p = P.DevicePolicy(env.observation_space, env.action_space, self.args, seed=12, critic=False)
        p.load_state_dict(self.sds[member])
        return p

    def league(self, **kw):
        if self.lg is None:
            self.lg = self.pkg.DeviceLeague(self.env, self.pool, episodes_per_env=K, **kw)
        return self.lg

    def stepwise(self, n_steps, deterministic=False):
        """The league's step from Python: the pool's whole-range launch, step_device, and the bookkeeping in torch."""
        env, pool, E, A = self.env, self.pool, self.E, self.A
        _, _, rew, done, info = env.device_tensors()
        cur = torch.cuda.current_stream()
        for _ in range(n_steps):
            pool.act_into_env(env, self.h, self.m, agents=slice(0, A), deterministic=deterministic, counter=pool.counter)
            pool.counter += 1
            env.step_device(stream=cur)
            dones_env = done.reshape(E, A).bool().all(dim=1)
            self.cum += rew.reshape(E, A)
            self.len += 1
            for e in torch.nonzero(dones_env).flatten().tolist():
                k = int(self.count[e])
                if k < K:
                    self.log_ret[e, k], self.log_len[e, k], self.log_end[e, k] = self.cum[e], self.len[e], self.t
                    self.log_code[e, k] = info.reshape(E, 4)[e, 1]
                    if k == K - 1:
                        self.remaining -= 1
                self.count[e] += 1
            self.cum[dones_env] = 0.0
            self.len[dones_env] = 0
            self.h.view(E, A, 1, 128)[dones_env] = 0.0
            masks = torch.ones(E, A, 1, device="cuda")
            masks[dones_env] = 0.0
            self.m.copy_(masks.reshape(-1, 1))
            self.t += 1

    def result(self, device):
        """everything that must agree; ``device``: the league's arrays, else the stepwise path's"""
        torch.cuda.synchronize()
        self.env.sync()
        n = lambda t: t.cpu().numpy()
        out = {"checksum": np.array(self.env.full_state_checksum(), dtype=np.uint64), "counter": np.array(self.pool.counter)}
        for name, t in zip(("act", "obs", "rew", "done", "info"), self.env.device_tensors()):
            out["env." + name] = n(t)
        names = ("log_returns", "log_lengths", "log_end_steps", "log_codes", "cum", "lengths", "counts", "states", "masks")
        mine = (self.log_ret, self.log_len, self.log_end, self.log_code, self.cum, self.len, self.count, self.h, self.m)
        for name, t in zip(names, mine):
            out[name] = n(self.lg.view(name) if device else t)
        out["members2"] = n(self.lg.view("members2")) if device else self.members2
        out["remaining"] = np.array(int(self.lg.view("remaining").item()) if device else self.remaining)
        out["steps"] = np.array(self.lg.steps if device else self.t)
        return out

    def close(self):
        for x in (self.lg, self.pool, self.env):
            if x is not None:
                x.close()


def bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def assert_same(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), k


LOG = ("log_returns", "log_lengths", "log_end_steps", "log_codes")


# ---- the sided launch
@pytest.mark.parametrize("case", list(CASES))
def test_sided_launch_matches_single_policies(pkg, P, case):
    s = Side(pkg, P, case)
    env, pool, E, A, nh = s.env, s.pool, s.E, s.A, s.nh
    half = A // 2
    assert CAP <= pool.num_tiles <= 2 * E * half // 32 + CAP and (case != "1v1" or pool.num_tiles == 2 * CAP)   # 1v1: two tiles a member
    s.stepwise(1)                                       # one env step: observations past the reset, non-zero states
    act_d = env.device_tensors()[0]
    side_member = np.repeat(s.members2, half, axis=1)   # [E, A]: the member of row (e, a)
    refs = [s.single(k) for k in range(CAP)]
    for det in (False, True):
        counter = 91 + det
        ho, lp = pool.act_into_env(env, s.h, s.m, agents=slice(0, A), deterministic=det, counter=counter, rnn_states_out=torch.empty_like(s.h))
        act_pool = act_d[:, :, :nh].clone()
        torch.cuda.current_stream().synchronize()
        assert ho.abs().max() > 0
        for k, ref in enumerate(refs):
            hr, lr = ref.act_into_env(env, s.h, s.m, agents=slice(0, A), deterministic=det, counter=counter, rnn_states_out=torch.empty_like(s.h))
            torch.cuda.current_stream().synchronize()
            sel = torch.as_tensor(side_member == k).cuda()                   # [E, A]
            assert sel.any() and not sel.all()
            tag = f"{case} det={det} member {k}"
            assert torch.equal(act_pool[sel], act_d[:, :, :nh][sel]), tag
            assert torch.equal(ho.view(E, A, 128)[sel], hr.view(E, A, 128)[sel]), tag
            assert torch.equal(lp.view(E, A)[sel], lr.view(E, A)[sel]), tag
    for r in refs:
        r.close()
    s.close()


# ---- run(n) against the stepwise loop
@pytest.mark.parametrize("case", ["1v1", "2v2"])
def test_run_equals_stepwise_loop(pkg, P, case):
    ref, dev = Side(pkg, P, case), Side(pkg, P, case)
    ref.stepwise(12)
    want = ref.result(False)
    # 12 steps fill every env's two slots, env 1 out of phase with the rest; states, sums and returns are not trivially zero
    assert (want["counts"] >= K).all() and want["remaining"] == 0 and (want["log_lengths"] > 0).all()
    assert want["log_end_steps"][1, 0] == 0 and len(set(want["log_end_steps"][:, 0].tolist())) > 1
    assert np.abs(want["states"]).max() > 0 and np.abs(want["log_returns"]).max() > 0
    assert (want["log_codes"] > 0).all() and (want["log_codes"][0] == TIMEOUT).all() and want["log_codes"][1, 0] != TIMEOUT
    lg = dev.league()
    assert lg.steps == -1
    lg.begin()
    assert lg.run(12) == 12 and lg.steps == 12
    got = dev.result(True)
    assert_same(got, want)
    assert dev.pool.counter == 82
    # five more steps: every env finishes a third episode, which is counted and leaves the log as it was
    ref.stepwise(5)
    lg.run(5)
    want17, got17 = ref.result(False), dev.result(True)
    assert_same(got17, want17)
    assert (got17["counts"] >= 3).all() and got17["remaining"] == 0
    for k in LOG:
        assert np.array_equal(bits(got17[k]), bits(got[k])), k
    # the table of that log: the host twin and the numpy restatement on the log copied back, and the same bytes from a second call
    tab = lg.table()
    logs = [got17[k] for k in ("log_returns", "log_lengths", "log_codes", "counts")]
    assert_table(tab, table_loop(*logs, dev.members2, CAP, 100.0))
    twin = pkg.league.table_host(*logs, dev.members2, CAP, 100.0)
    again = lg.table()
    for f in pkg.LeagueTable.FIELDS:
        assert np.array_equal(getattr(tab, f).view(np.uint8), getattr(twin, f).view(np.uint8)), f
        assert np.array_equal(getattr(tab, f).view(np.uint8), getattr(again, f).view(np.uint8)), f
    off = ~np.eye(CAP, dtype=bool)
    assert (tab.episodes[off] > 0).all() and (tab.episodes[~off] == 0).all() and tab.episodes.sum() == K * dev.E
    assert tab.steps.sum() == got17["log_lengths"].sum() and tab.timeouts.sum() == (got17["log_codes"] == TIMEOUT).sum()
    opp, mine, theirs = tab.against(0)
    assert opp.tolist() == [1, 2] and np.isfinite(mine).all() and np.isfinite(theirs).all()
    ref.close()
    dev.close()


def test_two_runs_equal_one_and_evaluate_stops_at_a_chunk_boundary(pkg, P):
    one, two = Side(pkg, P, "1v1"), Side(pkg, P, "1v1")
    a, b = one.league(), two.league()
    a.begin()
    a.run(12)
    b.begin()
    b.run(5)
    b.run(7)
    assert_same(two.result(True), one.result(True))
    # evaluate: env 1 fills its slots at steps 0 and 5, the others at steps 4 and 9, so remaining is 0 after 10 steps: chunks of 4 stop at 12
    for s in (one, two):
        s.reset()
        s.pool.counter = 70
    tab = a.evaluate(64, chunk=4)
    assert a.steps == 12 and a.remaining() == 0 and tab.episodes.sum() == K * one.E and one.pool.counter == 82
    b.begin()
    b.run(12)
    assert_same(two.result(True), one.result(True))
    # max_steps ends it early: 4 + 2 steps, quotas unfinished
    one.reset()
    tab6 = a.evaluate(6, chunk=4)
    assert a.steps == 6 and a.remaining() == one.E - 1 and tab6.episodes.sum() == one.E + 1
    with pytest.raises(ValueError, match="at least 1"):
        a.evaluate(0)
    one.close()
    two.close()


# ---- the table on synthetic values written through view()
def test_table_on_synthetic_log(pkg, P):
    s = Side(pkg, P, "1v1", E=70)                       # 70 envs: a cell's envs span more than one wave
    E, A, margin = s.E, s.A, 100.0
    lg = pkg.DeviceLeague(s.env, s.pool, episodes_per_env=3, win_margin=margin)
    s.lg = lg
    lg.begin()
    log_ret, log_len, log_code, count = threshold_log(E, 3, A, margin)
    cycle = [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2)]                       # cell (2, 1) and the diagonal stay empty; a cell's envs not adjacent
    m2 = np.array([cycle[e % len(cycle)] for e in range(E)], dtype=np.int32)
    m2[:7] = (0, 1)                                                        # the threshold episodes in one cell
    m2[69] = (0, 1)                                                        # and an env of that cell in the second wave
    count[69] = 5                                                          # count > K
    for name, arr in (("log_returns", log_ret), ("log_lengths", log_len), ("log_codes", log_code), ("counts", count), ("members2", m2)):
        lg.view(name).copy_(torch.as_tensor(arr).cuda())
    torch.cuda.synchronize()
    tab = lg.table()
    assert_table(tab, table_loop(log_ret, log_len, log_code, count, m2, CAP, margin))
    twin = pkg.league.table_host(log_ret, log_len, log_code, count, m2, CAP, margin)
    for f in pkg.LeagueTable.FIELDS:
        assert np.array_equal(getattr(tab, f).view(np.uint8), getattr(twin, f).view(np.uint8)), f
    assert tab.episodes[2, 1] == 0 and tab.sum_a[2, 1] == 0 and tab.wins_a[0, 1] >= 1 and tab.wins_b[0, 1] >= 1 and tab.draws[0, 1] >= 5
    # only the seven threshold episodes: exactly +-margin and inside are draws, the next float32 beyond each is a win
    one = np.zeros(E, dtype=np.int32)
    one[:7] = 1
    lg.view("counts").copy_(torch.as_tensor(one).cuda())
    torch.cuda.synchronize()
    t7 = lg.table()
    assert (t7.episodes[0, 1], t7.wins_a[0, 1], t7.wins_b[0, 1], t7.draws[0, 1]) == (7, 1, 1, 5) and t7.episodes.sum() == 7
    s.close()


# ---- refusals that need a device
def test_refusals_on_the_device(pkg, P):
    s = Side(pkg, P, "1v1", capacity=CAP + 1, pair=False)     # member 3 is never loaded
    env, pool, E, A, lib = s.env, s.pool, s.E, s.A, s.pkg.load_library()
    with pytest.raises(ValueError, match="no sided plan"):
        pkg.DeviceLeague(env, pool)
    pool.assign(np.zeros(E, dtype=np.int32), na=1)
    with pytest.raises(ValueError, match="no sided plan"):
        pkg.DeviceLeague(env, pool)
    # the per-env form's half-range call; a sided plan and its whole-range call in between; assign returns the pool to the per-env
    # form, and the same half-range call gives what it gave before
    rng = np.random.default_rng(5)
    h1 = torch.as_tensor(rng.normal(0, 0.5, (E, 1, 128)).astype(np.float32)).cuda()
    m1 = torch.ones(E, 1, device="cuda")
    members = (np.arange(E) % CAP).astype(np.int32)
    act_d = env.device_tensors()[0]

    def half_range():
        pool.assign(members, na=1)
        ho, lp = pool.act_into_env(env, h1, m1, agents=slice(1, 2), counter=33, rnn_states_out=torch.empty_like(h1))
        torch.cuda.synchronize()
        return ho.clone(), lp.clone(), act_d[:, 1].clone()

    before = half_range()
    assert before[0].abs().max() > 0
    pool.assign_sides(s.members2, A)
    pool.act_into_env(env, s.h, s.m, agents=slice(0, A), counter=34, rnn_states_out=torch.empty_like(s.h))
    for x, y in zip(half_range(), before):
        assert torch.equal(x, y)
    # a sided plan for another E, an odd A, K and the margin out of range
    pool.assign_sides(pkg.round_robin(E + 1, range(CAP)), A)
    with pytest.raises(ValueError, match="E differs"):
        pkg.DeviceLeague(env, pool)
    with pytest.raises(ValueError, match="even"):
        pool.assign_sides(s.members2, 3)
    pool.assign_sides(s.members2, A)
    for kw, what in ((dict(episodes_per_env=0), "episodes_per_env"), (dict(episodes_per_env=65), "episodes_per_env"),
                     (dict(win_margin=-1.0), "win_margin"), (dict(win_margin=float("nan")), "win_margin")):
        with pytest.raises(ValueError, match=what):
            pkg.DeviceLeague(env, pool, **kw)
    lg = pkg.DeviceLeague(env, pool, episodes_per_env=K)
    s.lg = lg
    with pytest.raises(ValueError, match="before ac_league_begin"):
        lg.run(1)
    with pytest.raises(ValueError, match="before ac_league_begin"):
        lg.table()
    # a half-range call and explicit rows on the sided pool, from Python and at the C ABI
    with pytest.raises(ValueError, match="sided plan"):
        pool.act_into_env(env, h1, m1, agents=slice(1, 2), counter=33)
    with pytest.raises(ValueError, match="sided plan"):
        pool.act(np.zeros((E, env.obs_dim), np.float32), np.zeros((E, 1, 128), np.float32), np.ones((E, 1), np.float32))
    rows = P.AcPolicyRows(E, 1, A, 1, env.act_dim)
    act, obs = env.device_tensors()[:2]
    lp2 = torch.zeros(E, 1, device="cuda")
    assert lib.ac_policy_pool_act(pool._h, pool._stream(), C.byref(rows), obs.data_ptr(), h1.data_ptr(), m1.data_ptr(), 0, 0, 0, act.data_ptr(),
                                  lp2.data_ptr(), h1.data_ptr()) == -1 and "sided plan" in lib.last_error()
    # a -1 side passes the plan's check and is refused by begin, with nothing written; so is a member that is not loaded
    m2 = s.members2.copy()
    m2[3, 1] = -1
    lg.pair(m2)
    with pytest.raises(ValueError, match="env 3 has side 1 assigned -1"):
        lg.begin()
    assert lg.steps == -1 and (lg.view("members2").cpu().numpy() == -1).all()
    m2[3, 1] = CAP
    with pytest.raises(ValueError, match="env 3"):
        lg.pair(m2)
    pool.assign_sides(m2, A, check=False)
    with pytest.raises(ValueError, match="env 3 has member 3 on side 1"):
        lg.begin()
    assert lg.steps == -1
    # a round, then the pool dealt again: run asks for a new begin; n_steps < 1
    lg.pair(s.members2)
    lg.begin()
    with pytest.raises(ValueError, match="n_steps"):
        lg.run(0)
    lg.run(2)
    lg.pair(s.members2)
    with pytest.raises(ValueError, match="assigned again"):
        lg.run(1)
    assert lg.steps == 2 and pool.counter == 72
    s.close()
