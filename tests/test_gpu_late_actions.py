"""The late-actions host step (ac_step_host_actions: header word, doorbell, copy, wait; csrc/late_actions.hpp and "Late actions" in
csrc/split_kernel.hpp) against a second handle of the same config and seed driven through step_async / step_wait, whose rows are plain
and in place before the launch. The kernel and its arithmetic are the same on both paths, so every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (8, 40)      # 16 aircraft: part of one workgroup; 80: two workgroups, the second with shadow tail lanes


def draw(rng, env):
    E, A = env.num_envs, env.num_agents
    return np.stack([rng.integers(0, k, size=(E, A)) for k in (41, 41, 41, 30)], axis=-1).astype(np.float32)


def late_stats(pkg, env):
    st = pkg.capi.AcLateStats()
    env.lib.check(env.lib.ac_late_stats(env._h, C.byref(st)), "ac_late_stats")
    return st


def configure(env, fraction=-1.0, budget=-1, delay_us=-1, timing=-1):
    env.lib.check(env.lib.ac_late_config(env._h, float(fraction), int(budget), int(delay_us), int(timing)), "ac_late_config")


def unpack(out):
    obs, rew, done, info = out
    return np.array(obs), np.array(rew), np.array(done), np.array(info._codes)


def assert_same_step(t, x, y):
    for k, name in enumerate(("obs", "rewards", "dones", "infos")):
        assert np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)), f"step {t}: {name} differ"


def plain_step(env, act):
    env.step_async(act)
    return env.step_wait()


def pair(pkg, n, max_steps=None):
    cfg = pkg.default_config("singlecombat")
    if max_steps:
        cfg.max_steps = max_steps
    a, b = pkg.HipVecEnv(cfg, n, seed=5), pkg.HipVecEnv(cfg, n, seed=5)
    a.reset(); b.reset()
    return a, b


def lockstep(pkg, a, b, rng, steps, keep=0, plain_actions=None, uses=None):
    """`a` through step() (late rows), `b` through step_async / step_wait (plain rows); the last `keep` results stay alive.
    `uses`: dict, set index -> the tags (0: plain rows) the set's header word held after each step into it"""
    held = []
    for t in range(steps):
        act = draw(rng, a)
        oa = a.step(act)
        if uses is not None:
            st = a._sets[a._cur]
            # the set's header block: one 64-byte line behind the action rows, which are padded to whole workgroups (ac_host_buffers)
            npad = (a.num_envs * a.num_agents + 63) // 64 * 64 * a.act_dim
            words = np.ctypeslib.as_array(C.cast(st["actions"].ctypes.data + (npad * 4 + 63) // 64 * 64, C.POINTER(C.c_int32)), shape=(3,))
            uses.setdefault(a._cur, []).append(int(words[0]))
        ob = plain_step(b, act if plain_actions is None else plain_actions(act))
        assert_same_step(t, unpack(oa), unpack(ob))
        held = (held + [(oa, ob)])[-keep:] if keep else []
        del oa, ob
    return held


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("keep", (0, 3))
def test_late_rows_step_bit_equal_to_plain_rows(pkg, n, keep):
    a, b = pair(pkg, n, max_steps=7)          # (auto-resets inside the window)
    rng = np.random.default_rng(21)
    # keep = 0: two sets alternate, 12 steps; keep = 3: the ring grows to four sets, 20 steps -- every set at least three times, both tags
    steps = 12 if keep == 0 else 20
    uses = {}
    held = lockstep(pkg, a, b, rng, steps, keep=keep, uses=uses)
    # every ring set at least three times, each with both tag values, alternating from one late use of a set to its next
    assert len(uses) == (4 if keep else 2), uses
    for k, tags in uses.items():
        late_tags = [t for t in tags if t != 0]
        assert len(tags) >= 3 and {1, 2} <= set(late_tags), (k, tags)
        assert all(x != y for x, y in zip(late_tags, late_tags[1:])), (k, tags)
    st = late_stats(pkg, a)
    assert st.last_late == 1 and st.steps == steps - 1, (st.steps, st.last_late)     # (the handle's first host step goes through HIP, rows plain)
    assert late_stats(pkg, b).steps == 0
    assert len(a._sets) == (4 if keep else 2)
    assert a.full_state_checksum() == b.full_state_checksum()
    del held
    a.close(); b.close()


@pytest.mark.parametrize("n", SIZES)
def test_a_delayed_copy_is_waited_for_and_counted(pkg, n):
    a, b = pair(pkg, n)
    rng = np.random.default_rng(22)
    lockstep(pkg, a, b, rng, 2)
    configure(a, fraction=1.0, delay_us=300)  # every row behind the doorbell, 300 us after it: the systems waves must ask again
    lockstep(pkg, a, b, rng, 6)
    st = late_stats(pkg, a)
    print(f"late steps {st.steps}, retries {st.retries}, last {st.last_retries}")
    assert st.last_late == 1 and st.retries > 0 and st.last_retries > 0
    assert a.full_state_checksum() == b.full_state_checksum()
    a.close(); b.close()


def test_an_exhausted_budget_fails_the_step_until_reset(pkg):
    n = 40
    a, b = pair(pkg, n)
    rng = np.random.default_rng(23)
    lockstep(pkg, a, b, rng, 4)               # (both sets have held tagged rows: a set's first late use after plain rows copies in front of the doorbell)
    configure(a, fraction=1.0, budget=5, delay_us=300)
    act = draw(rng, a)
    with pytest.raises(RuntimeError, match="retry budget"):
        a.step(act)
    with pytest.raises(RuntimeError, match="retry budget"):     # sticky until reset()
        a.step(act)
    configure(a, budget=pkg.capi.AC_LATE_BUDGET_DEFAULT, delay_us=0)
    b.close()
    fresh = pkg.HipVecEnv(pkg.default_config("singlecombat"), n, seed=5)
    oa, of = a.reset(), fresh.reset()
    assert np.array_equal(oa.view(np.uint8), of.view(np.uint8))
    lockstep(pkg, a, fresh, rng, 6)
    assert late_stats(pkg, a).last_late == 1
    assert a.full_state_checksum() == fresh.full_state_checksum()
    a.close(); fresh.close()


@pytest.mark.parametrize("n", SIZES)
def test_a_non_integer_throttle_index_loses_its_two_low_mantissa_bits(pkg, n):
    a, b = pair(pkg, n)
    rng = np.random.default_rng(24)
    lockstep(pkg, a, b, rng, 2)

    def cleared(act):
        out = act.copy()
        w = out[..., 3].view(np.uint32) & np.uint32(0xFFFFFFFC)
        out[..., 3] = w.view(np.float32)
        return out

    seen = 0
    for t in range(6):
        act = draw(rng, a)
        act[..., 3] = (rng.random(act.shape[:-1]) * 29.0).astype(np.float32)      # full 24-bit significands
        seen += int((act[..., 3].view(np.uint32) & 3 != 0).sum())
        oa, ob = a.step(act), plain_step(b, cleared(act))
        assert_same_step(t, unpack(oa), unpack(ob))
        del oa, ob
    assert seen > 0 and late_stats(pkg, a).last_late == 1
    assert a.full_state_checksum() == b.full_state_checksum()
    a.close(); b.close()


def test_steps_that_retry_as_a_rule_turn_the_late_order_off(pkg):
    """the self-check: a window of AC_LATE_WINDOW late steps of which more than AC_LATE_WINDOW_MAX_RETRY_STEPS retried moves a quarter of
    the batch back in front of the doorbell, the fourth such window puts the handle back on copy-first; ac_late_config with a share
    turns the late order on again"""
    a, b = pair(pkg, 8)
    rng = np.random.default_rng(25)
    lockstep(pkg, a, b, rng, 4)
    configure(a, fraction=1.0, delay_us=30)   # every step retries
    lockstep(pkg, a, b, rng, 1024)
    st = late_stats(pkg, a)
    assert st.lowered == 1 and st.fraction == 0.75 and st.disabled == 0 and st.retry_steps >= 1000, (st.lowered, st.fraction, st.retry_steps)
    lockstep(pkg, a, b, rng, 3 * 1024)        # a quarter less behind the doorbell per window, then copy-first
    st = late_stats(pkg, a)
    assert st.lowered == 4 and st.fraction == 0.0 and st.disabled == 1, (st.lowered, st.fraction, st.disabled)
    lockstep(pkg, a, b, rng, 4)
    after = late_stats(pkg, a)
    assert after.last_late == 0 and after.steps == st.steps
    configure(a, fraction=1.0, delay_us=0)
    lockstep(pkg, a, b, rng, 4)
    assert late_stats(pkg, a).last_late == 1 and late_stats(pkg, a).disabled == 0
    assert a.full_state_checksum() == b.full_state_checksum()
    a.close(); b.close()
