"""Spawn curricula on the MI355X (csrc/spawn_bank.hpp, spawn.py): a handle with a bank of reset templates against plain handles created
at the bank's spawns, env by env, on every path a handle steps through. max_steps = 3, so timeouts end every episode in lockstep and
eight steps cross two auto-resets; E = 5 is a partial workgroup, E = 40 with two aircraft two workgroups. The spawn kernel copies what
the init kernel wrote, so every comparison is on raw bytes."""
import ctypes as C
import importlib

import numpy as np
import pytest

import spawn_util as SU

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ANGLES = (0, 45, 90)
SEED = 12345                      # of the sample="upto" draws (test_spawn_host.py checks that it reaches every entry of three)


@pytest.fixture(scope="module")
def P(pkg):
    return importlib.import_module("aircombat-selfplay_amd.policy")


def config(pkg, task, angle=None, hierarchical=False):
    cfg = pkg.default_config(task, hierarchical=hierarchical)
    cfg.max_steps = 3
    if angle is not None:
        importlib.import_module("aircombat-selfplay_amd.config").apply_curriculum_spawn(cfg, angle)
    return cfg


def own_rows(pkg, cfg):
    """the handle's own cfg.init as a bank of one"""
    return [[pkg.AcInitState.from_buffer_copy(cfg.init[i]) for i in range(cfg.n_agents)]]


def pattern(E):
    return [(0, 1, 2, 1)[e % 4] for e in range(E)]


def write_stage(cur, values):
    cur.stage.copy_(torch.tensor(values, dtype=torch.int32))
    torch.cuda.synchronize()


def arrays(cur):
    cur._env.sync()
    torch.cuda.synchronize()
    return {k: getattr(cur, k).cpu().numpy() for k in SU.FIELDS}


def left(env, result=None, states=True):
    """what a step (or a reset) leaves behind: the device buffers, the host step's arrays, every aircraft's state vector"""
    env.sync()
    d = {n: t.cpu().numpy() for n, t in zip(("obs", "rew", "done", "info"), env.device_tensors()[1:])}
    if result is not None:
        obs, rew, done, infos = result
        d["h_obs"], d["h_rew"], d["h_done"], d["h_info"] = np.array(obs), np.array(rew), np.array(done), np.array(infos._codes)
    if states:
        d["state"] = np.stack([np.stack([env.get_state(e, a) for a in range(env.num_agents)]) for e in range(env.num_envs)])
    return d


def assert_handles_equal(a, b, t):
    assert set(a) == set(b)
    for k in a:
        assert SU.same(a[k], b[k]), (t, k)


def assert_envs_fly(got, plain, flown, now, t):
    """env e of `got` against env e of the plain handles: what the step computed (rewards, dones, info) is that of the entry it flew,
    what it left (observation, state) that of the entry it holds now -- the same entry unless the step reset the env"""
    for e in range(len(flown)):
        f, n = plain[flown[e]], plain[now[e]]
        for k in got:
            want = n if k in ("obs", "h_obs", "state") else f
            assert SU.same(got[k][e], want[k][e]), (t, e, k, flown[e], now[e])


def was_reset(d):
    flags = d["info"][:, 3] != 0
    assert flags.all() or not flags.any()            # timeouts end every episode in lockstep
    return bool(flags.all())


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("task", ["singlecombat", "scenario1", "scenario_nvn"])
def test_a_bank_of_one_is_invisible(pkg, task):
    cfg = config(pkg, task)
    a, b = pkg.HipVecEnv(cfg, 5, seed=7), pkg.HipVecEnv(cfg, 5, seed=7)
    cur = a.spawn_curriculum(init_states=own_rows(pkg, cfg))
    assert a.curriculum is cur and cur.attached and cur.num_entries == 1 and cur.histogram() == [5]
    assert SU.same(a.reset(), b.reset())
    rng = np.random.default_rng(1)
    resets = 0
    for t in range(8):
        act = SU.random_actions(rng, 5, a.num_agents, a.act_dim)
        la, lb = left(a, a.step(act), states=False), left(b, b.step(act), states=False)
        assert_handles_equal(la, lb, t)
        assert a.full_state_checksum() == b.full_state_checksum(), t
        resets += was_reset(la)
    assert resets == 2
    got = arrays(cur)
    assert got["spawned"].tolist() == [0] * 5 and got["episode"].tolist() == [3] * 5 and got["played"].tolist() == [2] * 5
    a.close(); b.close()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------

def plain_handles(pkg, task, E, seed=7):
    return [pkg.HipVecEnv(config(pkg, task, angle), E, seed=seed) for angle in ANGLES]


@pytest.mark.parametrize("task,E", [("scenario1", 5), ("scenario1", 40), ("scenario_nvn", 5)])
def test_each_env_flies_its_own_stage(pkg, task, E):
    env = pkg.HipVecEnv(config(pkg, task, 0), E, seed=7)
    plain = plain_handles(pkg, task, E)
    cur = env.spawn_curriculum(angles=ANGLES)
    st = pattern(E)
    write_stage(cur, st)
    obs = env.reset()
    got = dict(left(env), h_obs=obs)
    want = []
    for p in plain:
        obs = p.reset()
        want.append(dict(left(p), h_obs=obs))
    assert_envs_fly({k: got[k] for k in ("obs", "h_obs", "state")}, want, st, st, "reset")
    assert not SU.same(want[0]["obs"], want[1]["obs"]) and not SU.same(want[1]["state"], want[2]["state"])     # the spawns differ
    rng = np.random.default_rng(2)
    resets = 0
    for t in range(8):
        act = SU.random_actions(rng, E, env.num_agents, env.act_dim)
        got = left(env, env.step(act))
        want = [left(p, p.step(act)) for p in plain]
        assert_envs_fly(got, want, st, st, t)
        resets += was_reset(got)
    assert resets == 2
    a = arrays(cur)
    assert a["spawned"].tolist() == st and a["stage"].tolist() == st and a["episode"].tolist() == [3] * E
    assert cur.histogram() == [st.count(k) for k in range(3)]
    env.close()
    for p in plain:
        p.close()


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------

def test_a_stage_written_mid_episode_waits_for_the_reset(pkg):
    E = 5
    env = pkg.HipVecEnv(config(pkg, "scenario1", 0), E, seed=7)
    plain = plain_handles(pkg, "scenario1", E)
    cur = env.spawn_curriculum(angles=ANGLES)
    env.reset()
    for p in plain:
        p.reset()
    rng = np.random.default_rng(3)
    old, new = [0] * E, [0, 2, 0, 1, 2]
    for t in range(7):
        act = SU.random_actions(rng, E, 2, env.act_dim)
        got = left(env, env.step(act))
        want = [left(p, p.step(act)) for p in plain]
        if t < 2:
            assert not was_reset(got)
            assert_envs_fly(got, want, old, old, t)              # steps 1 and 2: the written stage disturbs nothing
        elif t == 2:
            assert was_reset(got)
            assert_envs_fly(got, want, old, new, t)              # step 3: the old angle's rewards and dones, the new angle's reset observation
        else:
            assert_envs_fly(got, want, new, new, t)
        if t == 0:
            write_stage(cur, new)
    assert arrays(cur)["spawned"].tolist() == new
    env.close()
    for p in plain:
        p.close()


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------

def test_the_auto_rule_on_the_device_equals_the_twin(pkg):
    E, steps = 5, 12
    cfg = config(pkg, "scenario1", 0)
    rng = np.random.default_rng(4)
    acts = [SU.random_actions(rng, E, 2, 8) for _ in range(steps)]
    # a dry run on an unattached handle: every env's first two episode returns, which decide whether it advances after them
    dry = pkg.HipVecEnv(cfg, E, seed=7)
    dry.reset()
    rets = np.zeros((4, E), dtype=np.float32)
    for t in range(steps):
        _, rew, _, _ = dry.step(acts[t])
        rets[t // 3] += np.array(rew)[:, 0, 0]
    dry.close()
    worst = np.sort(np.minimum(rets[0], rets[1]))
    assert worst[1] < worst[2]
    win_return = float((worst[1] + worst[2]) / 2)                # two envs miss it in one of their first two episodes, three do not
    env = pkg.HipVecEnv(cfg, E, seed=7)
    cur = env.spawn_curriculum(angles=ANGLES, mode="auto", win_return=win_return, window=2, win_rate=1.0)
    twin = SU.Twin(E, 3, 1, "auto", "at", 2, 2, np.float32(win_return))
    env.reset()
    twin.step(None, None, all_envs=True)
    for k, v in arrays(cur).items():
        assert SU.same(v, twin.arrays()[k]), ("reset", k)
    stages = []
    for t in range(steps):
        got = left(env, env.step(acts[t]), states=False)
        twin.step(got["rew"], got["info"])
        for k, v in arrays(cur).items():
            assert SU.same(v, twin.arrays()[k]), (t, k)
        stages.append(twin.stage.copy())
    assert (stages[5] == 1).sum() == 3 and (stages[5] == 0).sum() == 2      # on the twin: some envs advance after two episodes, some do not
    assert twin.episode.tolist() == [5] * E and np.abs(twin.return_sum).max() > 0
    env.close()


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------

def test_sample_upto_draws_the_entry_per_env_and_episode(pkg):
    E = 5
    env = pkg.HipVecEnv(config(pkg, "scenario1", 0), E, seed=7)
    plain = plain_handles(pkg, "scenario1", E)
    cur = env.spawn_curriculum(angles=ANGLES, sample="upto", seed=SEED)
    S = importlib.import_module("aircombat-selfplay_amd.spawn")
    write_stage(cur, [2, 2, 1, 2, 0])
    drawn = lambda ep: [S.draw(env.lib, SEED, e, ep, s) for e, s in enumerate([2, 2, 1, 2, 0])]
    assert [SU.draw(SEED, e, 1, 2) for e in range(E)] == [S.draw(env.lib, SEED, e, 1, 2) for e in range(E)]
    env.reset()
    for p in plain:
        p.reset()
    flown = arrays(cur)["spawned"].tolist()
    assert flown == drawn(1)
    seen = set(flown)
    rng = np.random.default_rng(5)
    ep = 1
    for t in range(8):
        act = SU.random_actions(rng, E, 2, env.act_dim)
        got = left(env, env.step(act))
        want = [left(p, p.step(act)) for p in plain]
        now = flown
        if was_reset(got):
            ep += 1
            now = arrays(cur)["spawned"].tolist()
            assert now == drawn(ep), (t, ep)
            seen |= set(now)
        assert_envs_fly(got, want, flown, now, t)
        flown = now
    assert ep == 3 and len(seen) > 1 and arrays(cur)["stage"].tolist() == [2, 2, 1, 2, 0]
    env.close()
    for p in plain:
        p.close()


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------

def path(env):
    return env.lib.ac_dispatch_path(env._h).decode()


def test_every_step_path_with_a_bank(pkg):
    E = 5
    envs = [pkg.HipVecEnv(config(pkg, "scenario1", 0), E, seed=7, copy=True) for _ in range(3)]
    curs = [e.spawn_curriculum(angles=ANGLES) for e in envs]
    for c in curs:
        write_stage(c, pattern(E))
    obs = [e.reset() for e in envs]
    assert SU.same(obs[0], obs[1]) and SU.same(obs[0], obs[2])
    a, b, c = envs
    d_act = c.device_tensors()[0]
    rng = np.random.default_rng(6)
    held = []
    for t in range(8):
        act = SU.random_actions(rng, E, 2, a.act_dim)
        ra = a.step(act)
        b.step_async(act)
        rb = b.step_wait()
        d_act.copy_(torch.from_numpy(act))
        c.step_device(stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        la, lb, lc = left(a, ra, states=False), left(b, rb, states=False), left(c, states=False)
        assert_handles_equal(la, lb, t)
        for k in lc:
            assert SU.same(lc[k], la[k]), (t, k)
            if k != "info":
                assert SU.same(lc[k], la["h_" + k]), (t, k)          # the host set holds what the device buffers hold, the respawned rows included
        assert a.full_state_checksum() == b.full_state_checksum() == c.full_state_checksum()
        held.append(ra)                                              # (the ring hands out further sets)
        assert path(a) == "hip: a spawn bank is attached"
    for x, y in zip(arrays(curs[0]).values(), arrays(curs[2]).values()):
        assert SU.same(x, y)
    a.stop_curriculum()
    assert a.curriculum is None and not curs[0].attached
    a.stop_curriculum()                                              # nothing attached: nothing happens
    for _ in range(2):
        a.step(SU.random_actions(rng, E, 2, a.act_dim))
    assert path(a) == "aql"
    with pytest.raises(ValueError, match="detached"):
        curs[0].stage
    for e in envs:
        e.close()


def attach_pattern(side):
    cur = side.env.spawn_curriculum(angles=ANGLES)
    write_stage(cur, pattern(side.env.num_envs))
    return cur


def test_device_rollout_with_a_bank_equals_the_stepwise_loop(pkg, P):
    import test_gpu_rollout_collect as T
    dev, step = T.Side(pkg, P, "hierarchical"), T.Side(pkg, P, "hierarchical")
    curs = [attach_pattern(s) for s in (dev, step)]
    assert dev.rollout().collect(8) == 8
    step.stepwise(8)
    T.assert_same(dev.result(True), step.result(False))
    got, want = arrays(curs[0]), arrays(curs[1])
    for k in SU.FIELDS:
        assert SU.same(got[k], want[k]), k
    assert got["spawned"].tolist() == pattern(T.E) and (got["episode"] >= 1).all()      # max_steps 5: every env has respawned from its entry
    dev.close()
    step.close()


def test_device_evaluator_with_a_bank_equals_the_stepwise_loop(pkg, P):
    import test_gpu_eval as TE
    dev, step = TE.Side(pkg, P, "hierarchical"), TE.Side(pkg, P, "hierarchical")
    curs = [attach_pattern(s) for s in (dev, step)]
    ev = dev.evaluator()
    ev.begin()
    assert ev.run(12) == 12
    step.stepwise(12)
    TE.assert_same(dev.result(True), step.result(False))
    got, want = arrays(curs[0]), arrays(curs[1])
    for k in SU.FIELDS:
        assert SU.same(got[k], want[k]), k
    assert got["spawned"].tolist() == pattern(TE.E) and (got["episode"] >= 2).all()
    dev.close()
    step.close()


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------------

def test_the_recorder_captures_the_respawned_aircraft(pkg):
    E = 5
    env = pkg.HipVecEnv(config(pkg, "scenario1", 0), E, seed=7)
    plain = plain_handles(pkg, "scenario1", E)
    rec = env.record(frames=8)
    cur = env.spawn_curriculum(angles=ANGLES)
    st = pattern(E)
    write_stage(cur, st)
    env.reset()
    for p in plain:
        p.reset()
    spawn_entity = [[[p.get_entity(e, a) for a in range(2)] for e in range(E)] for p in plain]     # each plain handle's aircraft at its spawn
    rng = np.random.default_rng(7)
    for t in range(3):
        env.step(SU.random_actions(rng, E, 2, env.act_dim))
    assert rec.count == 4
    u64 = lambda x: np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    for e in range(E):
        fr = rec.frames(e)
        assert fr["cur_step"][:, 0].tolist() == [0, 1, 2, 0]
        for f in (0, 3):                                             # the frame behind reset() and the frame of the step that auto-reset the env
            for a in range(2):
                assert np.array_equal(u64(fr["entity"][f, a]), u64(spawn_entity[st[e]][e][a])), (e, f, a)
    assert not np.array_equal(u64(spawn_entity[0][0][0]), u64(spawn_entity[1][0][0]))
    env.close()
    for p in plain:
        p.close()


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------------

def test_refusals_on_a_handle_change_nothing(pkg):
    cfg = config(pkg, "singlecombat")
    a, b = pkg.HipVecEnv(cfg, 5, seed=7), pkg.HipVecEnv(cfg, 5, seed=7)
    assert SU.same(a.reset(), b.reset())
    rng = np.random.default_rng(8)
    t = [0]

    def still_equal():
        act = SU.random_actions(rng, 5, 2, a.act_dim)
        assert_handles_equal(left(a, a.step(act), states=False), left(b, b.step(act), states=False), t[0])
        assert a.full_state_checksum() == b.full_state_checksum() and a.curriculum is None
        t[0] += 1

    rows = pkg.curriculum_bank(cfg, ANGLES)
    bad = pkg.curriculum_bank(cfg, ANGLES)
    bad[2][0].lat_geod_deg = 89.5
    one = own_rows(pkg, cfg)[0]
    for kw, msg in ((dict(init_states=bad), "bank entry 2, aircraft 0"), (dict(init_states=[]), "K must be in 1 .. 1024"),
                    (dict(init_states=[one] * 1025), "K must be in 1 .. 1024"), (dict(init_states=rows, window=33), "window must be in 1 .. 32"),
                    (dict(init_states=rows, window=4, win_rate=0.001), None), (dict(init_states=rows, mode="auto"), "needs win_return"),
                    (dict(init_states=rows, mode="auto", win_return=float("inf")), "finite win_return"), (dict(), "either angles= .* or init_states="),
                    (dict(angles=ANGLES, init_states=rows), "either angles= .* or init_states=")):
        if msg is None:                                              # ceil(0.001 * 4) = 1 win of 4: accepted, and taken off again
            a.spawn_curriculum(**kw)
            a.stop_curriculum()
        else:
            with pytest.raises(ValueError, match=msg):
                a.spawn_curriculum(**kw)
        still_equal()
    # a second bank on a handle that has one (a bank of one, which is invisible)
    cur = a.spawn_curriculum(init_states=own_rows(pkg, cfg))
    with pytest.raises(ValueError, match="already has a bank"):
        a.spawn_curriculum(angles=ANGLES)
    with pytest.raises(ValueError, match="window must be in 1 .. 32"):
        cur.set_config(window=40)
    assert a.curriculum is cur and cur.attached and cur.num_entries == 1
    a.stop_curriculum()
    still_equal()
    # the heading task has no template
    h = pkg.HipVecEnv(pkg.default_config("heading"), 3, seed=0)
    h2 = pkg.HipVecEnv(pkg.default_config("heading"), 3, seed=0)
    with pytest.raises(ValueError, match="no reset template"):
        h.spawn_curriculum(init_states=[[pkg.AcInitState.from_buffer_copy(h.config.init[0])]])
    assert SU.same(h.reset(), h2.reset())
    act = np.stack([rng.integers(0, n, size=(3, 1)) for n in (41, 41, 41, 30)], axis=-1).astype(np.float32)
    assert_handles_equal(left(h, h.step(act), states=False), left(h2, h2.step(act), states=False), "heading")
    for e in (a, b, h, h2):
        e.close()
