"""The device missile integrators held to the oracle tick by tick: ac_probe_missile runs the step kernels' own missile_run -- the
MslT<float> template and the MslD overload -- on the case groups of tests/missile_probe_util.py, one launch per group and (form,
parameter set) that a step kernel flies, on handles at the four battle-field centres, and every tick's munition record is compared
with the oracle's under that module's rules. The bounds come from the CPU twins and the primitives' recorded accuracy, never from the
device; tests/test_missile_probe_host.py shows the comparison failing for planted faults."""
import numpy as np
import pytest

import missile_probe_util as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def envs(pkg):
    made = {}

    def at(center):
        if center not in made:
            cfg = pkg.default_config("singlecombat")
            cfg.center_lat, cfg.center_lon, cfg.center_alt = center
            made[center] = pkg.HipVecEnv(cfg, 2, device_id=0)
        return made[center]
    yield at
    for e in made.values():
        e.close()


@pytest.mark.parametrize("name", list(M.GROUPS))
def test_device_missile_ticks_stay_within_their_bounds(envs, name):
    launch, target, center, combos = M.group(name)
    env = envs(center)
    verdicts = []
    for form, model in combos:
        got = env.probe_missile(form, model, launch, target)
        ok, worst, msg = M.compare(name, form, got)
        print(msg)
        verdicts.append((ok, msg))
    assert all(ok for ok, _ in verdicts), "\n".join(msg for ok, msg in verdicts if not ok)


def test_two_probe_runs_are_bit_identical(envs):
    launch, target, center, combos = M.group("over_top_9l")
    env = envs(center)
    for form, model in combos:
        a, b = env.probe_missile(form, model, launch, target), env.probe_missile(form, model, launch, target)
        assert a.tobytes() == b.tobytes(), form


def test_probe_refuses_bad_arguments_and_works_afterwards(envs, pkg):
    capi = pkg.capi
    launch, target, center, _ = M.group("golden_120b")
    env = envs(center)
    src = np.zeros((launch.shape[0], capi.AC_PROBE_MSL_IN))
    src[:] = launch
    tgt = np.ascontiguousarray(target[:8])
    dst = np.full((8, src.shape[0], capi.AC_PROBE_MSL_OUT), 7.0)
    good = (env._h, M.FP64, M.AIM120B, src.shape[0], 8, src.ctypes.data, tgt.ctypes.data, dst.ctypes.data)
    for what, i, bad in M.REFUSALS(capi):
        args = list(good)
        args[i] = bad
        assert env.lib.ac_probe_missile(*args) != 0, what
        assert env.lib.last_error().startswith("ac_probe_missile: "), (what, env.lib.last_error())
        assert (dst == 7.0).all(), what
    with pytest.raises(RuntimeError, match="ac_probe_missile failed: ac_probe_missile: unknown form"):
        env.probe_missile(2, M.AIM120B, launch, target[:8])
    got = env.probe_missile(M.FP64, M.AIM120B, launch, target[:8])
    assert (got[:, :, M.O_T] == (np.arange(8)[:, None] + 1.0) * (1.0 / 60.0)).all() and (got[:, :, M.O_MOVED] == 1.0).all()
