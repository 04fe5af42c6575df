"""VecEnv.step through the native entry (csrc/native_step.cpp) against the same step through ctypes (AIRCOMBAT_NATIVE_STEP=0): bit for bit
over every kernel form that takes host actions differently, the ownership rules of what step() returns, the inputs the native entry
hands back to Python, the library's errors, and two handles stepped from threads."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = 30


def make(pkg, monkeypatch, native, cfg, envs, **kw):
    """An env on the native step, or one pinned to the ctypes path."""
    if native:
        monkeypatch.delenv("AIRCOMBAT_NATIVE_STEP", raising=False)
    else:
        monkeypatch.setenv("AIRCOMBAT_NATIVE_STEP", "0")
    cls = pkg.HipShareVecEnv if cfg.n_agents > 2 else pkg.HipVecEnv
    env = cls(cfg, envs, **kw)
    monkeypatch.delenv("AIRCOMBAT_NATIVE_STEP", raising=False)
    assert (env._native is not None) == native, "the native step was not built" if native else "AIRCOMBAT_NATIVE_STEP=0 was not honoured"
    return env


def nvec(space):
    parts = getattr(space, "spaces", space if isinstance(space, tuple) else None)
    if parts is not None:
        return [n for s in parts for n in nvec(s)]
    return [int(n) for n in space.nvec] if hasattr(space, "nvec") else [int(space.n)]


def batches(env, count, seed=0):
    rng = np.random.default_rng(seed)
    ns = nvec(env.action_space)
    assert len(ns) == env.act_dim
    return [np.stack([rng.integers(0, n, size=(env.num_envs, env.num_agents)) for n in ns], axis=-1).astype(np.float32) for _ in range(count)]


def same(x, y):
    """bit-equal results: every array byte for byte, the info words too"""
    assert len(x) == len(y)
    for a, b in zip(x[:-1], y[:-1]):
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert x[-1]._codes.tobytes() == y[-1]._codes.tobytes()


CONFIGS = {
    "singlecombat": lambda pkg: (pkg.default_config("singlecombat"), 8),                         # the three-wave late-actions kernel
    "singlecombat_shoot": lambda pkg: (pkg.default_config("singlecombat_shoot"), 8),             # the quad form
    "scenario_nvn 2v2": lambda pkg: (pkg.default_config("scenario_nvn"), 4),                     # HipShareVecEnv: a five-tuple
    "hierarchical scenario1": lambda pkg: (pkg.default_config("scenario1", hierarchical=True), 4),   # the controller packet goes in front
}


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("copy", (True, False))
def test_bit_for_bit_against_the_ctypes_path(pkg, monkeypatch, name, copy):
    cfg, E = CONFIGS[name](pkg)
    nat = make(pkg, monkeypatch, True, cfg, E, seed=7, copy=copy)
    ref = make(pkg, monkeypatch, False, cfg, E, seed=7, copy=copy)
    r1, r2 = nat.reset(), ref.reset()
    assert np.asarray(r1[0] if cfg.n_agents > 2 else r1).tobytes() == np.asarray(r2[0] if cfg.n_agents > 2 else r2).tobytes()
    assert bool(nat.hierarchical) == name.startswith("hierarchical")
    for t, a in enumerate(batches(nat, STEPS)):
        x, y = nat.step(a), ref.step(a)
        same(x, y)
        assert nat._cur == ref._cur
        if cfg.n_agents > 2:
            assert len(x) == 5 and not x[1].flags.owndata and x[1].strides[1] == 0 and np.shares_memory(x[1], x[0])    # share_obs is still the view
        else:
            assert len(x) == 4
    if name == "singlecombat":       # (the form whose batch crosses under the launch: the native entry must be on that path, not beside it)
        st = pkg.capi.AcLateStats()
        nat.lib.check(nat.lib.ac_late_stats(nat._h, C.byref(st)), "ac_late_stats")
        assert st.steps == STEPS - 1 and st.last_late == 1, (st.steps, st.last_late)    # (a handle's first host step goes through HIP, rows plain)
    nat.close(); ref.close()


def test_ownership_of_what_step_returns(pkg, monkeypatch):
    cfg = pkg.default_config("singlecombat")
    nat = make(pkg, monkeypatch, True, cfg, 8, seed=3)
    ref = make(pkg, monkeypatch, False, cfg, 8, seed=3)
    nat.reset(); ref.reset()
    acts = iter(batches(nat, 64, seed=1))
    addr = lambda a: a.__array_interface__["data"][0]
    both = lambda: (lambda a: (nat.step(a), ref.step(a)))(next(acts))
    # keep step t's arrays and step twice more: they stay as they were, and the new results live in other sets
    kept, kref = both()
    frozen = [np.array(k) for k in kept[:3]] + [np.array(kept[3]._codes)]
    for _ in range(2):
        x, y = both()
        same(x, y)
        assert addr(x[0]) != addr(kept[0]) and not x[0].flags.owndata
        del x, y
    for k, f in zip(list(kept[:3]) + [kept[3]._codes], frozen):
        assert k.tobytes() == f.tobytes()
    same(kept, kref)
    # drop them: the set comes back into the ring, without a copy
    held = addr(kept[0])
    del kept, kref, k
    gc.collect()
    later = set()
    for _ in range(4):
        x, y = both()
        later.add(addr(x[0]))
        assert not x[0].flags.owndata
        del x, y
    assert held in later
    # hold more results than the ring has sets: the later ones are copies, with the values the ctypes path gives
    pairs = [both() for _ in range(pkg.vec_env.RING_SETS + 3)]
    assert sum(p[0][0].flags.owndata for p in pairs) == 3 and sum(p[1][0].flags.owndata for p in pairs) == 3
    assert len({addr(p[0][0]) for p in pairs}) == len(pairs)
    for x, y in pairs:
        same(x, y)
    assert len(nat._sets) == pkg.vec_env.RING_SETS and nat._native.n_sets == pkg.vec_env.RING_SETS
    del pairs, x, y
    gc.collect()
    x, y = both()                    # and the ring is in use again
    same(x, y)
    assert not x[0].flags.owndata
    del x, y
    nat.close(); ref.close()


def test_copy_false_alternates_the_two_sets(pkg, monkeypatch):
    cfg = pkg.default_config("singlecombat")
    env = make(pkg, monkeypatch, True, cfg, 8, seed=3, copy=False)
    env.reset()
    res = [env.step(a) for a in batches(env, 6)]
    assert all(res[i] is res[i % 2] for i in range(6)) and res[0] is not res[1]
    assert res[0] is env._results[1] and res[1] is env._results[0] and env._cur == 0
    env.close()


@pytest.mark.parametrize("form", ["nested lists", "float64", "strided slice", "read-only", "flat"])
def test_inputs_in_other_forms_give_the_same_results(pkg, monkeypatch, form):
    cfg = pkg.default_config("singlecombat")
    nat = make(pkg, monkeypatch, True, cfg, 8, seed=5)
    ref = make(pkg, monkeypatch, False, cfg, 8, seed=5)
    nat.reset(); ref.reset()

    def shaped(a):
        if form == "nested lists":
            return a.tolist()
        if form == "float64":
            return a.astype(np.float64)
        if form == "strided slice":
            wide = np.zeros(a.shape[:2] + (2 * a.shape[2],), dtype=np.float32)
            wide[:, :, ::2] = a
            v = wide[:, :, ::2]
            assert not v.flags.c_contiguous
            return v
        if form == "read-only":
            r = a.copy()
            r.flags.writeable = False
            return r
        return a.reshape(-1)

    for a in batches(nat, 6):
        x, y = nat.step(shaped(a)), ref.step(a)       # the reference env gets the plain array: the form must not matter
        same(x, y)
        assert not x[0].flags.owndata
        del x, y
    nat.close(); ref.close()


def test_a_wrong_size_raises_what_the_python_path_raises(pkg, monkeypatch):
    cfg = pkg.default_config("singlecombat")
    nat = make(pkg, monkeypatch, True, cfg, 8, seed=5)
    ref = make(pkg, monkeypatch, False, cfg, 8, seed=5)
    nat.reset(); ref.reset()
    a = batches(nat, 1)[0]
    for bad in (a[1:], np.concatenate([a, a]), a[1:].tolist()):
        with pytest.raises(Exception) as e_ref:
            ref.step(bad)
        with pytest.raises(Exception) as e_nat:
            nat.step(bad)
        assert type(e_nat.value) is type(e_ref.value) is ValueError
    same(nat.step(a), ref.step(a))                    # nothing was stepped, nothing is out of step
    nat.close(); ref.close()


def test_a_non_finite_state_raises_jsbsim_failed(pkg, monkeypatch):
    cfg = pkg.default_config("singlecombat")
    env = make(pkg, monkeypatch, True, cfg, 70, seed=3, copy=False)
    env.reset()
    acts = batches(env, 8)
    for a in acts[:3]:
        env.step(a)
    ix = env.lib.state_field_names().index("wq")
    st = env.get_state(37, 1)
    st[ix] = np.nan
    env.set_state(37, 1, st)
    with pytest.raises(RuntimeError) as err:
        for a in acts[3:6]:
            env.step(a)
    assert "JSBSim failed" in str(err.value) and "env 37, agent 1" in str(err.value) and str(err.value).startswith("ac_step_host_actions failed")
    assert env._results[env._cur][2][37, 1, 0]        # the step completed into the set the env calls current
    env.reset()
    assert np.isfinite(env.step(acts[6])[0]).all()
    env.close()


def test_step_after_close_raises_assertion_error(pkg, monkeypatch):
    env = make(pkg, monkeypatch, True, pkg.default_config("singlecombat"), 8)
    env.reset()
    a = batches(env, 1)[0]
    env.step(a)
    env.close()
    with pytest.raises(AssertionError):
        env.step(a)


def test_two_handles_stepped_from_threads_match_one(pkg, monkeypatch):
    monkeypatch.delenv("AIRCOMBAT_NATIVE_STEP", raising=False)
    cfg = pkg.default_config("singlecombat")
    E = 9
    many = pkg.MultiDeviceVecEnv(cfg, E, device_ids=[0, 0], seed=5)
    assert all(p._native is not None for p in many.parts) and [c for _, c in many.blocks] == [5, 4]
    one = make(pkg, monkeypatch, False, cfg, E, seed=5)
    assert many.reset().tobytes() == one.reset().tobytes()
    for a in batches(one, 10):
        same(many.step(a), one.step(a))
    many.close(); one.close()
