"""The device flight recorder (csrc/flight_recorder.hpp, recorder.py) on the MI355X: recorded frames against the host getters and the
files render() writes, on every path a handle steps through. Records are compared as raw bytes and files byte for byte: the capture
kernel runs the code ac_get_entity runs and copies the words ac_get_missile copies, so there is nothing to tolerate."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def P(pkg):
    return importlib.import_module("aircombat-selfplay_amd.policy")


def file_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def u64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def shoot_config(pkg):
    """test_render_writes_acmi_frames' config: close and nose-on, the shoot bit launches"""
    cfg = pkg.default_config("singlecombat_shoot")
    cfg.init[1].lon_deg, cfg.init[1].lat_geod_deg, cfg.init[1].psi_deg = 120.02, 60.06, 171.0
    return cfg


def shoot_actions(E):
    act = np.zeros((E, 2, 5), dtype=np.float32)
    act[..., :4] = [20, 18.6, 20, 15]
    act[..., 4] = 1
    return act


def rewind_render(env):
    """render()'s recording is not env state and restore() does not rewind it: start a new file"""
    env._acmi_started = False


def test_write_acmi_equals_render_1v1_missiles(pkg, tmp_path):
    env = pkg.HipVecEnv(shoot_config(pkg), 5)
    rec = env.record(envs=[0, 3, 4], frames=64)
    assert env.recorder is rec and rec.attached and rec.count == 0
    env.reset()
    want, got = str(tmp_path / "render.txt.acmi"), str(tmp_path / "rec.txt.acmi")
    act = shoot_actions(5)
    for _ in range(40):
        env.step(act)
        env.render(filepath=want, env=3)
    assert rec.count == 41                       # the reset and forty steps
    assert rec.write_acmi(got, env=3, first=1) == 40
    assert file_bytes(got) == file_bytes(want)
    assert b"Name=AIM-9L" in file_bytes(got)
    fr = rec.frames(3)
    assert fr.shape == (41, 2) and fr["flags"][0, 0] == 2 and not (fr["flags"][1:] & 2).any()
    assert fr["cur_step"][:2, 1].tolist() == [0, 1]
    env.close()


def test_write_acmi_equals_render_scenario_munitions_and_chaff(pkg, tmp_path):
    """test_render_scenario_munitions_and_chaff's flight, env 0 in the first pass and env 1 in a replay from the post-reset snapshot"""
    cfg = pkg.default_nvn_config(2, task="scenario_nvn")
    for i in range(4):
        cfg.init[i].lon_deg += 0.013 * (i % 3) + (0.02 if i >= 2 else 0.0)
        cfg.init[i].psi_deg = (7.0 + 3.0 * i) if i < 2 else (171.0 + 2.0 * i)
        if i >= 2:
            cfg.init[i].lat_geod_deg = 60.06
    env = pkg.HipShareVecEnv(cfg, 2, seed=3)
    rec = env.record(frames=160)
    env.reset()
    snap = env.snapshot(device=False)
    rng = np.random.default_rng(2)
    acts = []
    for step in range(140):
        act = np.zeros((2, 4, 8), dtype=np.float32)
        act[..., :4] = np.array([20, 18.6, 20, 15], dtype=np.float32) + rng.integers(-1, 2, size=(2, 4, 4))
        act[..., 4:] = rng.random((2, 4, 4)) < 0.7
        acts.append(act)
    want0, got0 = str(tmp_path / "render0.txt.acmi"), str(tmp_path / "rec0.txt.acmi")
    for act in acts:
        env.step(act)
        env.render(filepath=want0, env=0)
    assert rec.count == 141
    rec.write_acmi(got0, env=0, first=1)
    assert file_bytes(got0) == file_bytes(want0)
    text = open(got0, encoding="utf-8-sig").read().splitlines()
    assert any("Name=AIM-120B" in l for l in text)
    assert any(",Name=CHF,Color=" in l for l in text)
    assert any("Type=Misc+Explosion" in l and l.endswith("Radius=5") for l in text)
    # env 1 of the same flight: the recorder has it already; render() gets it from a replay
    env.stop_recording()
    assert env.recorder is None and not rec.attached
    env.restore(snap)
    rewind_render(env)
    want1, got1 = str(tmp_path / "render1.txt.acmi"), str(tmp_path / "rec1.txt.acmi")
    for act in acts:
        env.step(act)
        env.render(filepath=want1, env=1)
    assert rec.count == 141
    rec.write_acmi(got1, env=1, first=1)
    assert file_bytes(got1) == file_bytes(want1)
    env.close()


def test_write_acmi_across_an_auto_reset(pkg, tmp_path):
    cfg = pkg.default_config("singlecombat")
    env = pkg.HipVecEnv(cfg, 3, seed=0)
    rec = env.record(frames=400)
    rng = np.random.default_rng(1)
    env.seed(0)
    env.reset()
    snap = env.snapshot(device=False)
    acts, first_done = [], None
    for t in range(330):
        a = np.stack([rng.integers(0, n, size=(3, cfg.n_agents)) for n in (41, 41, 41, 30)], axis=-1).astype(np.float32)
        acts.append(a)
        _, _, d, _ = env.step(a)
        if first_done is None and d.any():
            first_done = int(np.nonzero(d.reshape(3, -1).any(axis=1))[0][0])
    assert first_done is not None and rec.count == 331
    e = first_done
    env.stop_recording()
    env.restore(snap)
    want, got = str(tmp_path / "render.txt.acmi"), str(tmp_path / "rec.txt.acmi")
    for a in acts:
        env.step(a)
        env.render(filepath=want, env=e)
    rec.write_acmi(got, env=e, first=1)
    assert file_bytes(got) == file_bytes(want)
    spans = rec.episodes(e)
    assert len(spans) >= 2 and spans[0][0] == 0 and spans[-1][1] == 330
    assert all(b[0] == a[1] + 1 for a, b in zip(spans, spans[1:]))
    for f, l in spans:
        assert rec.frames(e, f, l)["cur_step"][:, 0].tolist() == list(range(l - f + 1))
    # the step that ended the first episode reported done, and its frame already shows the next episode
    fr = rec.frames(e)
    assert (fr["flags"][spans[1][0]] & 1).all() and (fr["flags"][0] == 2).all()
    env.close()


WAVE_ENVS = [0, 1, 31, 32, 63, 64, 69]


def test_wave_edges_and_gather(pkg):
    """140 lanes: two full waves and a part; a gathered selection that straddles both wave edges"""
    E = 70
    env = pkg.HipVecEnv(shoot_config(pkg), E)
    A = env.record(frames=8)
    B = pkg.FlightRecorder(env, envs=WAVE_ENVS, frames=8)
    assert not B.attached and [c[0] for c in A.columns] == ["cur_step", "flags", "status", "entity", "msl_status", "msl_model", "msl_pose"]
    env.reset()
    B.capture(after_reset=True)
    act = shoot_actions(E)
    for _ in range(5):
        env.step(act)
        B.capture()
    assert A.count == 6 and B.count == 6
    names = env.lib.state_field_names()
    flying = 0
    for e in (0, 31, 32, 63, 64, 69):
        fa = A.frames(e)
        assert fa.shape == (6, 2) and fa.tobytes() == B.frames(e).tobytes()
        last = fa[-1]
        for a in range(2):
            assert np.array_equal(u64(last["entity"][a]), u64(env.get_entity(e, a))), (e, a)
            st = env.get_state(e, a)
            assert last["cur_step"][a] == 5 == int(st[names.index("cur_step")]) and last["status"][a] == int(st[names.index("status")])
            for k in range(4):
                m = env.get_missile(e, a, k)
                assert last["msl_status"][a, k] == int(m[0]) and last["msl_model"][a, k] == int(m[11]), (e, a, k)
                assert np.array_equal(u64(last["msl_pose"][a, k]), u64(m[[1, 2, 3, 7, 8]])), (e, a, k)
                flying += int(m[0]) == 0
    assert flying > 0                            # the slots compared hold munitions in flight
    # the torch view of the ring: [F, count, S, A], frame f in slot f % F
    env.sync()
    v = A.view("cur_step")
    assert tuple(v.shape) == (8, 1, E, 2) and (v[:6, 0].cpu().numpy() == np.arange(6)[:, None, None]).all() and not v[6:].any()
    assert tuple(B.view("msl_pose").shape) == (8, 20, len(WAVE_ENVS), 2)
    assert np.array_equal(u64(A.view("entity")[5, :, 64, 1].cpu().numpy()), u64(env.get_entity(64, 1)))
    env.close()


def test_single_aircraft_task_without_slots(pkg, tmp_path):
    cfg = pkg.default_config("heading")
    env = pkg.HipVecEnv(cfg, 3, seed=0)
    rec = env.record(frames=4)
    assert [c[0] for c in rec.columns] == ["cur_step", "flags", "status", "entity"] and rec.bytes_per_aircraft_frame == 108
    env.seed(0)
    env.reset()
    rng = np.random.default_rng(4)
    path = str(tmp_path / "render.txt.acmi")
    for _ in range(3):
        env.step(np.stack([rng.integers(0, n, size=(3, 1)) for n in (41, 41, 41, 30)], axis=-1).astype(np.float32))
        env.render(filepath=path, env=2)
    for e in range(3):
        fr = rec.frames(e)
        assert fr.shape == (4, 1) and fr["cur_step"][:, 0].tolist() == [0, 1, 2, 3]
        assert np.array_equal(u64(fr["entity"][-1, 0]), u64(env.get_entity(e, 0)))
    got = str(tmp_path / "rec.txt.acmi")
    rec.write_acmi(got, env=2, first=1)
    assert file_bytes(got) == file_bytes(path)
    env.close()


def test_ring_wrap(pkg):
    env = pkg.HipVecEnv(pkg.default_config("singlecombat"), 2)
    rec = env.record(frames=8)
    big = pkg.FlightRecorder(env, frames=16)
    env.reset()
    big.capture(after_reset=True)
    rng = np.random.default_rng(6)
    for _ in range(10):
        env.step(np.stack([rng.integers(0, n, size=(2, 2)) for n in (41, 41, 41, 30)], axis=-1).astype(np.float32))
        big.capture()
    assert rec.count == 11 and big.count == 11
    for e in range(2):
        assert rec.frames(e, 3, 10).tobytes() == big.frames(e, 3, 10).tobytes()
        assert rec.frames(e).tobytes() == big.frames(e, 3).tobytes() and rec.frames(e)["cur_step"][:, 0].tolist() == list(range(3, 11))
    with pytest.raises(ValueError, match="overwritten"):
        rec.frames(0, 2, 10)
    out = np.zeros(2 * rec.bytes_per_aircraft_frame, dtype=np.uint8)
    assert env.lib.ac_recorder_read(rec._h, 0, 2, 1, out.ctypes.data) == -1 and "overwritten" in env.lib.last_error() and not out.any()
    assert env.lib.ac_recorder_read(rec._h, 0, 10, 2, out.ctypes.data) == -1 and "not been captured" in env.lib.last_error()
    assert rec.count == 11 and rec.episodes(0) == [(3, 10)] and big.episodes(1) == [(0, 10)]
    env.close()


# ---- the three collectors ------------------------------------------------------------------------------------------------------------

def rings(side):
    return [side.rec.frames(e).tobytes() for e in range(side.env.num_envs)]


def test_evaluator_records_and_its_log_does_not_change(pkg, P, tmp_path):
    import test_gpu_eval as TE
    sides = [TE.Side(pkg, P, "selfplay_policy", episodes_per_env=4) for _ in range(3)]
    dev, step, plain = sides
    for s in sides:
        s.rec = s.env.record(frames=32) if s is not plain else None
        s.env.reset()                                # the recorded handles capture this reset: frame 0
        for ag in range(s.A):
            s.env.set_status(1, ag, 1)
    ev, ev_plain = dev.evaluator(), plain.evaluator()
    ev.begin()
    ev.run(24)
    ev_plain.begin()
    ev_plain.run(24)
    step.stepwise(24)
    got, want = dev.result(True), plain.result(True)
    TE.assert_same(got, want)
    assert dev.rec.count == 25 == step.rec.count and rings(dev) == rings(step)
    res = ev.result()
    assert res.logged.all() and len(set(res.end_steps[:, 0].tolist())) > 1      # four episodes per env, env 1 out of phase
    for e in range(TE.E):
        for k in range(4):
            L = int(res.lengths[e, k])
            first, last = ev.episode_frames(e, k)
            assert last - first + 1 == L and first == 1 + int(res.end_steps[e, k]) - L
            assert dev.rec.frames(e, first, last)["cur_step"][:, 0].tolist() == list(range(L))
            path = str(tmp_path / f"ep_{e}_{k}.acmi")
            assert ev.write_episode_acmi(path, e, k) == L
            assert sum(l.startswith("#") for l in open(path, encoding="utf-8-sig").read().splitlines()) == L
    with pytest.raises(ValueError, match="no logged episode"):
        ev.episode_frames(0, 4)
    with pytest.raises(ValueError, match="no flight recorder"):
        ev_plain.episode_frames(0, 0)
    for s in sides:
        s.close()


def test_evaluator_refuses_episodes_that_left_the_ring_or_began_unrecorded(pkg, P):
    import test_gpu_eval as TE
    s = TE.Side(pkg, P, "selfplay_policy", episodes_per_env=4)
    rec = s.env.record(frames=12)                    # attached after the reset: the first episode's reset state was never recorded
    ev = s.evaluator()
    ev.begin()
    ev.run(24)
    with pytest.raises(ValueError, match="before recording did"):
        ev.episode_frames(0, 0)
    with pytest.raises(ValueError, match="overwritten"):
        ev.episode_frames(0, 1)
    with pytest.raises(ValueError, match="overwritten"):
        ev.episode_frames(0, 2)                      # frames 9 .. 13, of which 12 .. 23 are left
    first, last = ev.episode_frames(0, 3)
    assert (first, last) == (14, 18) and rec.frames(0, first, last)["cur_step"][:, 0].tolist() == [0, 1, 2, 3, 4]
    s.close()


@pytest.mark.parametrize("which", ["ppo", "mappo"])
def test_rollout_collectors_record_and_their_buffers_do_not_change(pkg, P, which):
    T = importlib.import_module("test_gpu_rollout_collect" if which == "ppo" else "test_gpu_rollout_share")
    sides = [T.Side(pkg, P, "1v1") for _ in range(3)]
    dev, step, plain = sides
    for s in (dev, step):
        s.rec = s.env.record(frames=32)
    for window in range(3):                          # 3 x 8 = 24 steps from C++
        assert dev.rollout().collect() == T.T and plain.rollout().collect() == T.T
        step.stepwise(T.T)
        T.assert_same(dev.result(True), plain.result(True))
        for s in sides:
            s.buffer.after_update()
    assert dev.rec.count == 24 == step.rec.count and rings(dev) == rings(step)
    fr = dev.rec.frames(0)
    assert fr["cur_step"][:, 0].tolist() == [(t + 1) % 5 for t in range(24)]      # max_steps 5: episodes inside the window
    for s in sides:
        s.close()


# ---- host steps and refusals -----------------------------------------------------------------------------------------------------------

def test_host_steps_with_a_recorder(pkg):
    cfg = pkg.default_config("singlecombat")
    a, b = pkg.HipVecEnv(cfg, 4, seed=5), pkg.HipVecEnv(cfg, 4, seed=5)
    rec = a.record(envs=[1, 3], frames=16)
    assert np.array_equal(a.reset(), b.reset())
    rng = np.random.default_rng(8)
    acts = [np.stack([rng.integers(0, n, size=(4, 2)) for n in (41, 41, 41, 30)], axis=-1).astype(np.float32) for _ in range(9)]
    for t in range(6):
        ra, rb = a.step(acts[t]), b.step(acts[t])
        for x, y in zip(ra[:3], rb[:3]):
            assert x.tobytes() == y.tobytes(), t
    assert rec.count == 7
    for e in (1, 3):
        fr = rec.frames(e, 1, 6)
        assert fr["cur_step"][:, 0].tolist() == [1, 2, 3, 4, 5, 6]
        assert np.array_equal(u64(fr["entity"][-1, 1]), u64(a.get_entity(e, 1)))
    a.stop_recording()
    for t in range(6, 9):
        ra, rb = a.step(acts[t]), b.step(acts[t])
        for x, y in zip(ra[:3], rb[:3]):
            assert x.tobytes() == y.tobytes(), t
    assert rec.count == 7 and rec.frames(3)["cur_step"][:, 0].tolist() == list(range(7))
    a.close()
    b.close()


def test_refusals_change_nothing(pkg):
    cfg = pkg.default_config("singlecombat")
    env, other = pkg.HipVecEnv(cfg, 4), pkg.HipVecEnv(cfg, 4)
    lib = env.lib
    rec = env.record(envs=[0, 2], frames=4)
    env.reset()
    env.step(np.zeros((4, 2, 4), dtype=np.float32) + np.array([20, 18.6, 20, 15], dtype=np.float32))
    state = lambda: (rec.count, rec.frames(0).tobytes(), rec.frames(2).tobytes(), env.recorder is rec, rec.attached)
    before = state()
    assert before[0] == 2
    for sel, msg in (([2, 0], "not sorted"), ([1, 1], "appears twice"), ([0, 4], "out of range"), ([-1, 0], "out of range"), ([], "S must be in 1"),
                     ([0, 1, 2, 3, 3], "S must be in 1")):
        with pytest.raises(ValueError, match=msg):
            pkg.FlightRecorder(env, envs=sel)
    with pytest.raises(ValueError, match="at least 1 frame"):
        pkg.FlightRecorder(env, frames=0)
    with pytest.raises(ValueError, match="at least 1 frame"):
        env.record(envs=[1], frames=-3)
    # a recorder made for another handle
    foreign = pkg.FlightRecorder(other, frames=2)
    with pytest.raises(ValueError, match="made for another handle"):
        foreign.attach(env)
    assert not foreign.attached and foreign.count == 0
    # a second recorder on a handle that has one
    with pytest.raises(ValueError, match="already has a recorder"):
        env.record(frames=2)
    # an env that is not selected, through Python and at the C ABI
    with pytest.raises(ValueError, match="not among the recorded envs"):
        rec.frames(1)
    out = np.zeros(2 * rec.bytes_per_aircraft_frame, dtype=np.uint8)
    assert lib.ac_recorder_read(rec._h, 1, 0, 1, out.ctypes.data) == -1 and "not among the recorded envs" in lib.last_error() and not out.any()
    # an allocation the runtime refuses: 2^31 - 1 frames of 8 aircraft are 1.8 TB
    with pytest.raises(ValueError, match="ac_recorder_create"):
        pkg.FlightRecorder(env, frames=2 ** 31 - 1)
    n = C.c_int64()
    assert lib.ac_recorder_bytes(env._h, 4, 2 ** 31 - 1, C.byref(n)) == 0 and n.value > 10 ** 12
    assert lib.ac_recorder_bytes(env._h, 2, 4, C.byref(n)) == 0 and n.value == rec.nbytes
    assert state() == before
    env.step(np.zeros((4, 2, 4), dtype=np.float32) + np.array([20, 18.6, 20, 15], dtype=np.float32))
    assert rec.count == 3 and rec.frames(2)["cur_step"][:, 0].tolist() == [0, 1, 2]
    env.close()
    other.close()
