"""Snapshot, restore and clone of the env state (include/aircombat.h: ac_snapshot_*, ac_clone_envs; HipVecEnv.snapshot / restore /
clone_envs), on the device. Every comparison is exact: a restored or cloned env must continue bit for bit as the original did."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E = 64


def make_cfg(pkg, task, per_side=1, hierarchical=False, max_steps=60):
    if task == "heading":
        cfg = pkg.default_config("heading")
    elif per_side == 1:
        cfg = pkg.default_config(task, hierarchical=hierarchical)
        if task != "singlecombat":          # close and nose-on: munitions fly within a few steps
            cfg.init[1].lon_deg, cfg.init[1].lat_geod_deg, cfg.init[1].psi_deg = 120.02, 60.06, 171.0
            cfg.init[0].psi_deg = 9.0
    else:
        cfg = pkg.default_nvn_config(per_side, task=task, hierarchical=hierarchical)
        for i in range(2 * per_side):
            cfg.init[i].lon_deg += 0.013 * (i % 3) + (0.02 if i >= per_side else 0.0)
            cfg.init[i].psi_deg = (7.0 + 3.0 * i) if i < per_side else (171.0 + 2.0 * i)
            cfg.init[i].h_sl_ft += 300.0 * i
            if i >= per_side:
                cfg.init[i].lat_geod_deg = 60.06
    cfg.max_steps = max_steps               # episodes end inside the replayed window: the auto-reset runs after a restore
    return cfg


def make_env(pkg, cfg, n=E, seed=5, **kw):
    cls = pkg.HipShareVecEnv if cfg.n_agents > 2 else pkg.HipVecEnv
    return cls(cfg, n, seed=seed, **kw)


def actions(rng, env, weapons=True):
    return draw(rng, env.num_envs, env.num_agents, env.act_dim, env.hierarchical, weapons)


def draw(rng, n, A, d, hierarchical, weapons=True):
    if hierarchical:
        a = np.stack([rng.integers(0, k, size=(n, A)) for k in (3, 5, 3)], axis=-1)
    else:
        a = (np.array([20, 18.6, 20, 15]) + rng.integers(-3, 4, size=(n, A, 4)))
    a = a.astype(np.float32)
    if d > a.shape[-1]:
        a = np.concatenate([a, (rng.random((n, A, d - a.shape[-1])) < (0.5 if weapons else -1.0)).astype(np.float32)], axis=-1)
    return a


def obs_of(out):
    return out[0] if isinstance(out, tuple) else out


def run(env, acts):
    """step through `acts`; per step: obs, rewards, dones, info codes and the full-state digest"""
    rec = []
    for a in acts:
        out = env.step(a)
        obs, rew, done, info = (out[0], out[2], out[3], out[4]) if len(out) == 5 else out
        rec.append((np.array(obs), np.array(rew), np.array(done), np.array(info._codes), env.full_state_checksum()))
    return rec


def assert_same(r1, r2):
    assert len(r1) == len(r2)
    ended = False
    for t, (x, y) in enumerate(zip(r1, r2)):
        for k, name in enumerate(("obs", "rewards", "dones", "infos")):
            assert np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)), f"step {t}: {name} differ"
        assert x[4] == y[4], f"step {t}: full-state digest differs"
        ended |= bool(x[2].any())
    return ended


def chaff_seen(env):
    """has any aircraft released chaff (its remaining count below the config's, as tests/test_gpu_parity.py counts releases)?"""
    ix = env._ix("x_rem_chaff")
    return any(env.get_state(e, a)[ix] < env.config.num_missiles[a] for e in range(env.num_envs) for a in range(env.num_agents))


# every kernel form a BASELINE config launches (ac_create picks it from the task and the grid; AIRCOMBAT_SPLIT / AIRCOMBAT_QUAD pin it)
CASES = {
    "singlecombat_three_wave": ("singlecombat", 1, False, {"AIRCOMBAT_SPLIT": "1"}),
    "singlecombat_one_wave": ("singlecombat", 1, False, {"AIRCOMBAT_SPLIT": "0"}),
    "shoot_pair": ("singlecombat_shoot", 1, False, {"AIRCOMBAT_QUAD": "0"}),
    "shoot_quad": ("singlecombat_shoot", 1, False, {"AIRCOMBAT_QUAD": "1"}),
    "dodge_quad": ("singlecombat_dodge_missile", 1, False, {}),
    "scenario1": ("scenario1", 1, False, {}),
    "scenario1_hierarchical": ("scenario1", 1, True, {}),
    "scenario_2v2": ("scenario_nvn", 2, False, {}),
    "scenario_2v2_hierarchical": ("scenario_nvn", 2, True, {}),
    "scenario_4v4": ("scenario_nvn", 4, False, {}),
    "scenario_4v4_hierarchical": ("scenario_nvn", 4, True, {}),
    "heading": ("heading", 1, False, {}),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_round_trip_is_bit_exact(pkg, monkeypatch, case):
    task, per_side, hier, pins = CASES[case]
    for k, v in pins.items():
        monkeypatch.setenv(k, v)
    max_steps = {"heading": 25, "scenario1": 90, "scenario_nvn": 330}.get(task, 60)   # (releases come late: tests/test_gpu_parity.py flies 330 steps)
    env = make_env(pkg, make_cfg(pkg, task, per_side, hier, max_steps=max_steps))
    if task == "heading":
        env.seed(11)                         # ac_seed_envs: numpy's PCG64 streams are part of the state
    env.reset()
    rng = np.random.default_rng(3)
    munitions = task not in ("singlecombat", "heading")
    # the NvN scenarios are snapshotted after chaff releases; the 1v1 closing geometry releases none (its missiles are decided before
    # one comes within the 1000 m chaff range: none in 322 steps of 64 envs; tests/test_gpu_parity.py asks chaff of the NvN tasks only)
    scenario = task == "scenario_nvn"
    k, out = 0, None
    while k < max_steps - 8:                 # snapshot while munitions fly (and, for the scenario tasks, after chaff releases)
        out = env.step(actions(rng, env))
        k += 1
        if k >= 5 and (not munitions or (env.munitions_in_flight() > 0 and (not scenario or chaff_seen(env)))):
            break
    if munitions:
        assert env.munitions_in_flight() > 0
    if scenario:
        assert chaff_seen(env), "no chaff released before the snapshot"
    snap = env.snapshot()
    digest = env.full_state_checksum()
    obs_then = np.array(out[0])
    m = max_steps - k + 6
    acts = [actions(rng, env) for _ in range(m)]
    first = run(env, acts)
    obs = obs_of(env.restore(snap))
    assert env.full_state_checksum() == digest
    assert np.array_equal(obs.view(np.uint8), obs_then.view(np.uint8))
    second = run(env, acts)
    assert assert_same(first, second), "no episode ended inside the replayed window"
    env.close()


def test_restore_returns_the_snapshot_observation(pkg):
    env = make_env(pkg, make_cfg(pkg, "singlecombat"))
    env.reset()
    rng = np.random.default_rng(0)
    for _ in range(3):
        out = env.step(actions(rng, env))
    want = np.array(out[0])
    snap = env.snapshot(device=False)
    for _ in range(4):
        env.step(actions(rng, env))
    got = env.restore(snap)
    assert np.array_equal(got, want)
    env.close()


@pytest.mark.parametrize("task,per_side,hier", [("singlecombat_shoot", 1, False), ("scenario_nvn", 2, True), ("heading", 1, False)])
def test_restore_into_fresh_handle_through_bytes(pkg, task, per_side, hier):
    """the resume case: a checkpoint's bytes restored into a new handle made from the same config continue like the original"""
    cfg = make_cfg(pkg, task, per_side, hier, max_steps=30)
    env = make_env(pkg, cfg)
    if task == "heading":
        env.seed(4)
    env.reset()
    rng = np.random.default_rng(9)
    for _ in range(12):
        env.step(actions(rng, env))
    blob = env.snapshot().to_bytes()
    acts = [actions(rng, env) for _ in range(25)]
    first = run(env, acts)
    env.close()
    fresh = make_env(pkg, cfg)
    snap = pkg.EnvSnapshot.from_bytes(blob, expect=fresh)
    fresh.restore(snap)
    assert assert_same(first, run(fresh, acts))
    fresh.close()


@pytest.mark.parametrize("task,per_side,hier", [("singlecombat", 1, False), ("singlecombat_shoot", 1, False), ("heading", 1, False),
                                                ("scenario_nvn", 2, True)])
def test_clone_one_env_into_many(pkg, task, per_side, hier):
    cfg = make_cfg(pkg, task, per_side, hier, max_steps=40)
    env = make_env(pkg, cfg)
    ref = make_env(pkg, cfg)
    for x in (env, ref):
        if task == "heading":
            x.seed(2)
        x.reset()
    rng = np.random.default_rng(1)
    for _ in range(8):
        a = actions(rng, env)
        env.step(a)
        ref.step(a)
    src, dst = 5, np.array([0, 9, 17, 40, 63])
    env.clone_envs([src] * len(dst), dst)
    others = np.setdiff1d(np.arange(E), dst)
    for t in range(30):
        a = actions(rng, env, weapons=task != "scenario_nvn")   # (no launches: the scenario tasks' decoy draws are keyed by env index)
        a[dst] = a[src]                       # identical actions for the clones and their source
        o1, o2 = env.step(a), ref.step(a)
        obs1, rew1 = obs_of(o1), (o1[2] if len(o1) == 5 else o1[1])
        obs2, rew2 = obs_of(o2), (o2[2] if len(o2) == 5 else o2[1])
        for d in dst:                         # every clone flies like its source...
            assert np.array_equal(obs1[d], obs1[src]), f"step {t}: env {d}"
            assert np.array_equal(rew1[d], rew1[src]), f"step {t}: env {d}"
        assert np.array_equal(obs1[others], obs2[others]), f"step {t}"   # ... and the envs not named are untouched
        assert np.array_equal(rew1[others], rew2[others]), f"step {t}"
    env.close()
    ref.close()


def test_bad_requests_are_refused_and_change_nothing(pkg):
    cfg = make_cfg(pkg, "singlecombat_shoot")
    env = make_env(pkg, cfg)
    env.reset()
    rng = np.random.default_rng(2)
    for _ in range(5):
        env.step(actions(rng, env))
    digest = env.full_state_checksum()
    with pytest.raises(ValueError, match="appears twice"):
        env.clone_envs([1, 2], [3, 3])
    with pytest.raises(ValueError, match="out of range"):
        env.clone_envs([1], [E])
    with pytest.raises(ValueError, match="out of range"):
        env.clone_envs([-1], [0])
    with pytest.raises(ValueError, match="both a source"):
        env.clone_envs([0, 1], [1, 2])                        # a chain
    with pytest.raises(ValueError, match="both a source"):
        env.clone_envs([1, 2], [2, 1])                        # a swap
    other_e = make_env(pkg, cfg, n=E // 2)
    other_cfg = make_env(pkg, make_cfg(pkg, "singlecombat_shoot", max_steps=61))
    other_task = make_env(pkg, make_cfg(pkg, "singlecombat"))
    for o in (other_e, other_cfg, other_task):
        o.reset()
        with pytest.raises(ValueError):
            env.restore(o.snapshot())
        with pytest.raises(ValueError):
            env.restore(o.snapshot(device=False), envs=[0])
    assert env.full_state_checksum() == digest
    # the C ABI refuses them too, with the reason in ac_last_error
    import ctypes as C
    snap = other_e.snapshot()
    assert env.lib.ac_snapshot_load(env._h, C.c_void_p(snap.data.data_ptr())) != 0
    assert "number of envs" in env.lib.last_error()
    assert env.full_state_checksum() == digest
    for o in (env, other_e, other_cfg, other_task):
        o.close()


def test_decoy_seed_mismatch_is_refused(pkg):
    """the scenario tasks' decoy draws hang off the handle's seed: a snapshot only resumes under the seed it was taken with"""
    cfg = make_cfg(pkg, "scenario1")
    a, b = make_env(pkg, cfg, seed=5), make_env(pkg, cfg, seed=6)
    a.reset(), b.reset()
    digest = b.full_state_checksum()
    with pytest.raises(ValueError, match="config_hash"):
        b.restore(a.snapshot())
    assert b.full_state_checksum() == digest
    a.close(), b.close()


def test_controller_precision_mismatch_is_refused(pkg):
    cfg = make_cfg(pkg, "scenario_nvn", 2, True)
    fast = make_env(pkg, cfg, controller_precision="fast")
    fp32 = make_env(pkg, cfg, controller_precision="fp32")
    fast.reset(), fp32.reset()
    digest = fp32.full_state_checksum()
    with pytest.raises(ValueError, match="ctl_precision|config_hash"):
        fp32.restore(fast.snapshot())
    assert fp32.full_state_checksum() == digest
    fast.close(), fp32.close()


def records(env, envs):
    """ac_get_state / ac_get_missile of every aircraft (and munition slot) of `envs`"""
    slots = env.snapshot_header()["msl_slots"]
    return {(e, a): (env.get_state(e, a), [env.get_missile(e, a, k) for k in range(slots)]) for e in envs for a in range(env.num_agents)}


def assert_records(got, want, what):
    for key, (st, ms) in want.items():
        assert np.array_equal(got[key][0], st), f"{what}: state of env {key[0]} agent {key[1]}"
        for k, m in enumerate(ms):
            assert np.array_equal(got[key][1][k], m), f"{what}: munition {k} of env {key[0]} agent {key[1]}"


@pytest.mark.parametrize("task,per_side,hier,device", [("singlecombat_shoot", 1, False, True), ("singlecombat_shoot", 1, False, False),
                                                       ("scenario_nvn", 4, True, True)])
def test_partial_restore(pkg, task, per_side, hier, device):
    """restore(snap, envs=idx) against references that do not use the partial path: what env idx held at snapshot time (its outputs,
    ac_get_state, ac_get_missile, and the continuation of a handle restored WHOLE from that time), and what a run that never restored
    holds for every other env"""
    cfg = make_cfg(pkg, task, per_side, hier)
    env, ref, twin = make_env(pkg, cfg), make_env(pkg, cfg), make_env(pkg, cfg)
    env.reset(), ref.reset()
    rng = np.random.default_rng(6)
    for _ in range(6):
        a = actions(rng, env)
        out = env.step(a)
        ref.step(a)
    idx = np.array([2, 3, 31, 50])
    others = np.setdiff1d(np.arange(E), idx)
    obs_then = np.array(obs_of(out))
    then = records(env, idx)
    snap = env.snapshot(device=device)
    twin.restore(env.snapshot(device=False))                  # (whole-batch load: ac_snapshot_load_host)
    for _ in range(7):
        a = actions(rng, env)
        env.step(a)
        out = ref.step(a)
    obs_now = np.array(obs_of(out))
    obs = obs_of(env.restore(snap, envs=idx))
    assert np.array_equal(obs[idx], obs_then[idx])            # the restored envs hand back their snapshot-time observation ...
    assert np.array_equal(obs[others], obs_now[others])       # ... the others their current one
    assert_records(records(env, idx), then, "restored env")
    sample = [0, 1, 4, 30, 32, 63]
    assert_records(records(env, sample), records(ref, sample), "untouched env")
    for t in range(10):                                       # the continuation: idx like the twin, the rest like the reference
        a = actions(rng, env)
        o, r, w = obs_of(env.step(a)), obs_of(ref.step(a)), obs_of(twin.step(a))
        assert np.array_equal(o[idx], w[idx]), f"step {t}"
        assert np.array_equal(o[others], r[others]), f"step {t}"
    for x in (env, ref, twin):
        x.close()


def test_device_snapshot_is_ordered_for_other_readers(pkg):
    """a device snapshot taken behind queued steps is read on other streams -- to_bytes (torch's stream) and a restore into another
    handle (that handle's stream) -- before the saving handle is synchronised: both must see the finished copy"""
    cfg = make_cfg(pkg, "singlecombat_shoot", max_steps=2000)
    n = 4096
    a, b = make_env(pkg, cfg, n=n), make_env(pkg, cfg, n=n)
    a.reset(), b.reset()
    a.snapshot_header()                                       # (the first header reads the reset template: a host wait)
    for _ in range(30):                                       # queued, not waited for
        a.step_device()
    snap = a.snapshot()
    blob = snap.to_bytes()
    b.restore(snap)
    a.sync()
    want = a.snapshot(device=False)
    assert np.array_equal(np.frombuffer(blob, dtype=np.uint8), want.data)
    assert b.full_state_checksum() == a.full_state_checksum()
    a.close(), b.close()


def test_clone_is_ordered_on_torch_stream(pkg):
    import torch
    cfg = make_cfg(pkg, "singlecombat")
    dev, host = make_env(pkg, cfg), make_env(pkg, cfg)
    dev.reset(), host.reset()
    rng = np.random.default_rng(8)
    a1, a2 = actions(rng, dev), actions(rng, dev)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t1 = torch.from_numpy(a1).cuda()
        dev.step_device(t1.data_ptr(), stream=s)
        src = torch.tensor([4, 4, 7], dtype=torch.int32, device="cuda")
        dst = torch.tensor([10, 11, 12], dtype=torch.int32, device="cuda")
        dev.lib.check(dev.lib.ac_order_after(dev._h, s.cuda_stream), "ac_order_after")
        dev.clone_envs(src, dst)
        t2 = torch.from_numpy(a2).cuda()
        dev.step_device(t2.data_ptr(), stream=s)
    s.synchronize()
    host.step(a1)
    host.clone_envs([4, 4, 7], [10, 11, 12])
    host.step(a2)
    dev.sync()
    assert dev.full_state_checksum() == host.full_state_checksum()
    obs = dev.device_tensors()[1].cpu().numpy()
    assert np.array_equal(obs, host._restored_obs())
    dev.close(), host.close()


def test_multi_device_round_trip(pkg):
    cfg = make_cfg(pkg, "scenario_nvn", 2, False)
    env = pkg.MultiDeviceVecEnv(cfg, 32, [0, 0], seed=3)
    env.reset()
    rng = np.random.default_rng(4)
    step = lambda: env.step(draw(rng, 32, env.num_agents, env.act_dim, False))
    for _ in range(5):
        step()
    snap = env.snapshot()
    rng_state = rng.bit_generator.state
    first = [np.array(step()[0]) for _ in range(8)]
    env.restore(snap)
    rng.bit_generator.state = rng_state
    second = [np.array(step()[0]) for _ in range(8)]
    for x, y in zip(first, second):
        assert np.array_equal(x, y)
    blob = snap.to_bytes()
    back = pkg.MultiSnapshot.from_bytes(blob)
    env.restore(back)
    rng.bit_generator.state = rng_state
    assert np.array_equal(np.array(step()[0]), first[0])
    env.close()
