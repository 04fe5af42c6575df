"""The opponent pool's host side (no GPU): the plan (a stable sort of the call's rows by member, then tiles of <= 32 rows of one member)
through its host twin, the refusals of creation, assignment and member copies, and the member sizes."""
import importlib

import numpy as np
import pytest

import policy_util as U

P = importlib.import_module("aircombat-selfplay_amd.policy")
ve = importlib.import_module("aircombat-selfplay_amd.vec_env")


def _cfg(tag="a", precision="fast", **kw):
    a = U.args(tag)
    a.__dict__.update(kw)
    obs, act = U.spaces(tag)
    return P.make_config(obs, act, a, precision)


def _check_plan(members, na, cap, loaded=None):
    members = np.asarray(members, dtype=np.int32)
    E = members.size
    order, tiles, bad = P.plan_host(members, na, cap, loaded)
    ok = np.ones(cap, bool) if loaded is None else np.asarray(loaded, bool)
    valid = (members >= 0) & (members < cap)
    valid[valid] &= ok[members[valid]]
    # a numpy stable argsort of the valid envs by member, expanded to their rows
    envs = np.nonzero(valid)[0]
    envs = envs[np.argsort(members[envs], kind="stable")]
    want = (envs[:, None] * na + np.arange(na)[None, :]).ravel()
    assert np.array_equal(order[:want.size], want)
    # every assigned row exactly once, no other
    assert np.array_equal(np.sort(order[:want.size]), np.sort(np.nonzero(np.repeat(valid, na))[0]))
    # tiles: one member each, 1 .. 32 rows, member-major, covering the sorted rows in order without gaps
    pos = 0
    for m, p0, p1 in tiles:
        assert p0 == pos and 0 < p1 - p0 <= 32
        rows = order[p0:p1]
        assert (members[rows // na] == m).all()
        pos = p1
    assert pos == want.size
    counts = np.bincount(members[valid], minlength=cap) * na
    assert len(tiles) == int(np.sum((counts + 31) // 32))
    bad_envs = np.nonzero((members != -1) & ~valid)[0]
    assert bad == (int(bad_envs[0]) if bad_envs.size else -1)
    return order, tiles, bad


def _split(E, ids):
    m = np.empty(E, np.int32)
    for k, idx in enumerate(np.array_split(np.arange(E), len(ids))):
        m[idx] = ids[k]
    return m


@pytest.mark.parametrize("na", [1, 2])
@pytest.mark.parametrize("E,cap,seed", [(1, 1, 0), (31, 3, 1), (33, 8, 2), (1000, 5, 3), (4096, 16, 4), (777, 300, 5)])
def test_plan_random_assignments(E, cap, seed, na):
    rng = np.random.default_rng(seed)
    _check_plan(rng.integers(0, cap, E), na, cap)
    # with -1 entries (envs not acted for)
    m = rng.integers(-1, cap, E)
    _check_plan(m, na, cap)


@pytest.mark.parametrize("na", [1, 2])
@pytest.mark.parametrize("E,K", [(4096, 1), (4096, 8), (100, 3), (16384, 16), (5, 8)])
def test_plan_array_split(E, K, na):
    cap = max(K, 2)
    order, tiles, _ = _check_plan(_split(E, list(range(K))), na, cap)
    # the array_split ranges are contiguous and in member order, so the plan keeps the call's row order
    assert np.array_equal(order, np.arange(E * na))
    # reversed member ids: the sort moves the ranges
    m = _split(E, list(range(K))[::-1])
    order, _, _ = _check_plan(m, na, cap)
    if K > 1 and E >= K:
        assert not np.array_equal(order, np.arange(E * na))


@pytest.mark.parametrize("na", [1, 2])
@pytest.mark.parametrize("E", [1, 32, 33, 97, 1024])
def test_plan_all_one_member(E, na):
    _, tiles, _ = _check_plan(np.full(E, 2), na, 4)
    assert (tiles[:, 0] == 2).all() and len(tiles) == (E * na + 31) // 32


def test_plan_all_unassigned():
    order, tiles, bad = _check_plan(np.full(50, -1), 1, 3)
    assert len(tiles) == 0 and bad == -1


def test_plan_flags_bad_members():
    m = np.array([0, 1, 5, 1, -3, 0], np.int32)   # 5: out of range for capacity 3, -3: below -1
    _, _, bad = _check_plan(m, 1, 3)
    assert bad == 2
    # an unloaded member is flagged too, and its envs are left out like -1
    m = np.array([0, 1, 2, 1, 0, 2], np.int32)
    order, tiles, bad = _check_plan(m, 2, 3, loaded=[1, 0, 1])
    assert bad == 1
    assert set(tiles[:, 0]) == {0, 2}


def test_plan_max_tiles_bounds_the_count():
    rng = np.random.default_rng(9)
    lib = P.load_library()
    import ctypes as C
    for E, na, cap in [(1, 1, 1), (33, 2, 7), (4096, 1, 16), (100, 2, 300)]:
        mt = C.c_int64()
        lib.check(lib.ac_policy_pool_max_tiles(E, na, cap, C.byref(mt)), "max_tiles")
        for _ in range(5):
            _, tiles, _ = P.plan_host(rng.integers(0, cap, E), na, cap)
            assert len(tiles) <= mt.value


def test_member_sizes_are_the_actor_blob():
    import ctypes as C
    lib = P.load_library()
    for tag in ("a", "b"):
        for precision in ("fast", "fp32"):
            cfg = _cfg(tag, precision)
            na, _ = P.check_config(cfg)
            ns, npk = C.c_int64(), C.c_int64()
            lib.check(lib.ac_policy_pool_member_floats(C.byref(cfg), P.AC_POOL_PPO, 4, C.byref(ns), C.byref(npk)), "member_floats")
            assert ns.value == na
            assert npk.value > ns.value   # two or three 16-bit pieces per weight
    # the MAPPO form: the actor part of ac_policy_mappo_blob_floats
    import mappo_util as M
    for tag in ("a", "b"):
        o, c, act = M.spaces(tag)
        mc = P.make_mappo_config(o, c, act, M.args(tag))
        na, _ = P.check_mappo_config(mc)
        ns, npk = C.c_int64(), C.c_int64()
        lib.check(lib.ac_policy_pool_member_floats(C.byref(mc.base), P.AC_POOL_MAPPO, 2, C.byref(ns), C.byref(npk)), "member_floats")
        assert ns.value == na


def test_refusals_capacity_and_config():
    import ctypes as C
    lib = P.load_library()
    ns, npk = C.c_int64(), C.c_int64()
    cfg = _cfg()
    for cap in (0, -1):
        assert lib.ac_policy_pool_member_floats(C.byref(cfg), P.AC_POOL_PPO, cap, C.byref(ns), C.byref(npk)) != 0
        assert "capacity" in lib.last_error()
    # DevicePolicyPool refuses before any device is touched, UnsupportedPolicy by name
    obs, act = U.spaces("a")
    with pytest.raises(P.UnsupportedPolicy, match="capacity"):
        P.DevicePolicyPool(obs, act, U.args("a"), 0)
    with pytest.raises(P.UnsupportedPolicy, match="use_prior"):
        P.DevicePolicyPool(obs, act, U.args("a").__class__(**{**U.args("a").__dict__, "use_prior": False}), 2)
    with pytest.raises(P.UnsupportedPolicy, match="obs_dim"):
        P.DevicePolicyPool(ve._Box(-10, 10, (65,)), act, U.args("a"), 2)   # the PPO form takes obs_dim <= 32
    with pytest.raises(ValueError, match="form"):
        P.DevicePolicyPool(obs, act, U.args("a"), 2, form="qmix")


def test_refusals_copy_from():
    base = _cfg("a")
    assert P.pool_compatible(base, "ppo", _cfg("a"), "ppo") is None
    # a learner with a critic copies its actor: has_critic does not matter
    c = _cfg("a")
    c.has_critic = 1
    assert P.pool_compatible(base, "ppo", c, "ppo") is None
    assert "form" in P.pool_compatible(base, "ppo", _cfg("a"), "mappo")
    assert "precision" in P.pool_compatible(base, "ppo", _cfg("a", "fp32"), "ppo")
    assert "configuration" in P.pool_compatible(base, "ppo", _cfg("b"), "ppo")
    assert "configuration" in P.pool_compatible(base, "ppo", _cfg("a", use_feature_normalization=True), "ppo")
