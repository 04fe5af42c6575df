"""Host steps dispatched as AQL packets on the handle's own queue (csrc/aql_dispatch.hpp) against a twin handle pinned to the HIP runtime's
launch (AIRCOMBAT_DISPATCH=hip), made with the same config and seed. The kernels and their argument bytes are the same on both paths, so
every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def draw(rng, env):
    E, A, d = env.num_envs, env.num_agents, env.act_dim
    if env.hierarchical:
        a = np.stack([rng.integers(0, k, size=(E, A)) for k in (3, 5, 3)], axis=-1)
    else:
        a = np.stack([rng.integers(0, k, size=(E, A)) for k in (41, 41, 41, 30)], axis=-1)
    a = a.astype(np.float32)
    if d > a.shape[-1]:
        a = np.concatenate([a, (rng.random((E, A, d - a.shape[-1])) < 0.3).astype(np.float32)], axis=-1)
    return a


def path(env):
    return env.lib.dll.ac_dispatch_path(env._h).decode()


def twins(pkg, monkeypatch, cfg, n, seed=7, **kw):
    cls = pkg.HipShareVecEnv if cfg.n_agents > 2 else pkg.HipVecEnv
    monkeypatch.delenv("AIRCOMBAT_DISPATCH", raising=False)
    a = cls(cfg, n, seed=seed, **kw)
    monkeypatch.setenv("AIRCOMBAT_DISPATCH", "hip")
    b = cls(cfg, n, seed=seed, **kw)
    monkeypatch.delenv("AIRCOMBAT_DISPATCH", raising=False)
    assert path(b) == "AIRCOMBAT_DISPATCH=hip"
    return a, b


def unpack(out):
    obs, rew, done, info = (out[0], out[2], out[3], out[4]) if len(out) == 5 else out
    return np.array(obs), np.array(rew), np.array(done), np.array(info._codes)


def assert_same_step(t, x, y):
    for k, name in enumerate(("obs", "rewards", "dones", "infos")):
        assert np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)), f"step {t}: {name} differ"


def lockstep(a, b, rng, steps, keep=3):
    """step both twins with the same actions; the last `keep` results stay alive, so the default mode's ring hands out several sets"""
    held = []
    for t in range(steps):
        act = draw(rng, a)
        oa, ob = a.step(act), b.step(act)
        assert_same_step(t, unpack(oa), unpack(ob))
        held = (held + [(oa, ob)])[-keep:]
    return held


CONFIGS = {   # name: (config factory, envs, environment of the form)
    "c2_4096_three_wave": (lambda p: p.default_config("singlecombat"), 4096, {}),
    "singlecombat_one_wave": (lambda p: p.default_config("singlecombat"), 4096, {"AIRCOMBAT_SPLIT": "0"}),
    "heading": (lambda p: p.default_config("heading"), 512, {}),
    "legacy_2v2": (lambda p: p.default_config("multiplecombat_shoot"), 256, {}),
    "scenario1_quad": (lambda p: p.default_config("scenario1"), 512, {"AIRCOMBAT_QUAD": "1"}),
    "scenario_nvn_4v4": (lambda p: p.default_nvn_config(2, task="scenario_nvn"), 256, {}),
    "hierarchical_singlecombat": (lambda p: p.default_config("singlecombat", hierarchical=True), 512, {}),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_aql_host_steps_match_the_hip_path_bit_for_bit(pkg, monkeypatch, name):
    make, n, env_vars = CONFIGS[name]
    for k, v in env_vars.items():
        monkeypatch.setenv(k, v)
    cfg = make(pkg)
    cfg.max_steps = 120                   # auto-resets inside the window
    a, b = twins(pkg, monkeypatch, cfg, n)
    a.reset(); b.reset()
    assert path(a) == "pending"
    rng = np.random.default_rng(11)
    lockstep(a, b, rng, 300)
    assert path(a) == "aql", path(a)
    assert len(a._sets) > 2               # (the ring grew: more than one host set went through the AQL path)
    assert a.full_state_checksum() == b.full_state_checksum()
    a.close(); b.close()


def test_entry_points_between_async_aql_steps_keep_the_twins_equal(pkg, monkeypatch):
    cfg = pkg.default_config("singlecombat_shoot")
    cfg.max_steps = 80
    a, b = twins(pkg, monkeypatch, cfg, 256)
    a.reset(); b.reset()
    rng = np.random.default_rng(3)
    lockstep(a, b, rng, 5)
    assert path(a) == "aql"
    import torch
    dev = [torch.from_numpy(draw(rng, a)).cuda() for _ in range(4)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()

    def both(f):
        return f(a), f(b)

    for t in range(40):
        act = draw(rng, a)
        for e in (a, b):
            e.step_async(act)
        # entry points called while the AQL step may still be in flight: each waits for it first
        k = t % 6
        if k == 0:
            x, y = both(lambda e: e.get_state(t % 256, 1))
            assert np.array_equal(x, y)
        elif k == 1:
            sa, sb = both(lambda e: e.snapshot())
        elif k == 2:
            x, y = both(lambda e: e.full_state_checksum())
            assert x == y
        elif k == 3:
            for e in (a, b):
                e.lib.check(e.lib.ac_order_before(e._h, C.c_void_p(side.cuda_stream)), "ac_order_before")
        x, y = unpack(a.step_wait()), unpack(b.step_wait())
        assert_same_step(t, x, y)
        if k == 4:
            for e in (a, b):
                e.step_device(dev[t % 4].data_ptr())
            for e in (a, b):
                e.sync()
        elif k == 5 and t > 10:
            for e, s in ((a, sa), (b, sb)):
                e.restore(s)
        if t == 20:
            a.reset(); b.reset()
    lockstep(a, b, rng, 10)
    assert path(a) == "aql"
    assert a.full_state_checksum() == b.full_state_checksum()
    a.close(); b.close()


def test_a_reallocated_host_set_rebuilds_its_kernargs(pkg, monkeypatch):
    cfg = pkg.default_config("singlecombat")
    a, b = twins(pkg, monkeypatch, cfg, 256, copy=False)
    a.reset(); b.reset()
    rng = np.random.default_rng(5)
    lockstep(a, b, rng, 4, keep=1)
    assert path(a) == "aql"
    lib = a.lib.dll
    # give set 0 up and allocate it again: new host buffers behind the same set index (the kernarg block of the set must follow them)
    ptrs = {}
    for e in (a, b):
        old = [C.c_void_p() for _ in range(5)]
        e.lib.check(lib.ac_host_buffers(e._h, 0, *[C.byref(p) for p in old]), "ac_host_buffers")
        e.lib.check(lib.ac_host_set_detach(e._h, 0), "ac_host_set_detach")
        new = [C.c_void_p() for _ in range(5)]
        e.lib.check(lib.ac_host_buffers(e._h, 0, *[C.byref(p) for p in new]), "ac_host_buffers")
        ptrs[id(e)] = (old, new)
    for e in (a, b):
        old, new = ptrs[id(e)]
        E, A = e.num_envs, e.num_agents
        act = np.ctypeslib.as_array(C.cast(new[0], C.POINTER(C.c_float)), shape=(E * A * e.act_dim,))
        act[:] = draw(np.random.default_rng(9), e).ravel()
        e.lib.check(lib.ac_step_host(e._h, 0), "ac_step_host")
    oa = [np.ctypeslib.as_array(C.cast(ptrs[id(a)][1][k], C.POINTER(t)), shape=(s,)).copy()
          for k, t, s in ((1, C.c_float, 256 * 2 * a.obs_dim), (2, C.c_float, 512), (4, C.c_int32, 256))]
    ob = [np.ctypeslib.as_array(C.cast(ptrs[id(b)][1][k], C.POINTER(t)), shape=(s,)).copy()
          for k, t, s in ((1, C.c_float, 256 * 2 * b.obs_dim), (2, C.c_float, 512), (4, C.c_int32, 256))]
    assert np.abs(oa[0]).sum() > 0            # the step wrote into the new buffers
    for x, y in zip(oa, ob):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert path(a) == "aql"
    for e in (a, b):
        e._sets[0]["owner"].detached = True     # (the old buffers are the caller's now: freed with the arrays that view them)
    assert a.full_state_checksum() == b.full_state_checksum()
    a.close(); b.close()


def test_host_steps_inside_a_timing_bracket_go_through_hip(pkg, monkeypatch):
    cfg = pkg.default_config("singlecombat")
    monkeypatch.delenv("AIRCOMBAT_DISPATCH", raising=False)
    env = pkg.HipVecEnv(cfg, 1024, seed=1)
    env.reset()
    rng = np.random.default_rng(2)
    for _ in range(3):
        env.step(draw(rng, env))
    assert path(env) == "aql"
    lib = env.lib.dll
    ev = C.c_float()
    st, _ = env._hand_over(draw(rng, env))
    env.lib.check(env.lib.ac_timing_begin(env._h), "ac_timing_begin")
    env.lib.check(lib.ac_step_host_async(env._h, st["index"]), "ac_step_host_async")
    env.lib.check(env.lib.ac_timing_end(env._h, C.byref(ev)), "ac_timing_end")
    # the events bracket the step kernel on the stream: an AQL dispatch would leave them nothing to time
    assert ev.value > 0.005, ev.value
    env.lib.check(lib.ac_step_host_wait(env._h), "ac_step_host_wait")
    assert path(env) == "aql"
    env.step(draw(rng, env))
    env.close()


def test_a_non_finite_state_is_reported_through_the_aql_path(pkg, monkeypatch):
    cfg = pkg.default_config("singlecombat")
    a, b = twins(pkg, monkeypatch, cfg, 70, copy=False)
    a.reset(); b.reset()
    rng = np.random.default_rng(1)
    lockstep(a, b, rng, 3, keep=1)
    assert path(a) == "aql"
    ix = a.lib.state_field_names().index("wq")
    for e in (a, b):
        st = e.get_state(37, 1)
        st[ix] = np.nan
        e.set_state(37, 1, st)
    msgs = []
    act = draw(rng, a)
    for e in (a, b):
        with pytest.raises(RuntimeError) as err:
            for _ in range(3):
                e.step(act)
        msgs.append(str(err.value))
    assert "JSBSim failed" in msgs[0] and "env 37, agent 1" in msgs[0], msgs[0]
    assert msgs[0].replace("ac_step_host", "") == msgs[1].replace("ac_step_host", "")
    assert path(a) == "aql"
    a.close(); b.close()
