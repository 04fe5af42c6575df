"""The device math primitives, each held to its own bound: ac_probe_math runs the inline functions the step kernels call on the input sets of
tests/math_probe_util.py, and the results are compared with that module's references (bit for bit with its float32 twins for the ops
that only add, compare and take remainders). The bounds come from the CPU twins and the hardware approximations' documented accuracy
(math_probe_util.py), never from the device; tests/test_math_probe_host.py shows the comparison failing for planted faults."""
import ctypes as C

import numpy as np
import pytest

import math_probe_util as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(pkg):
    cfg = pkg.default_config("singlecombat")
    assert (cfg.center_lat, cfg.center_lon, cfg.center_alt) == M.CENTER     # the centre the geodesy references are about
    e = pkg.HipVecEnv(cfg, 2, device_id=0)
    yield e
    e.close()


@pytest.mark.parametrize("op", M.OPS)
def test_device_primitive_stays_within_its_bound(env, op):
    got = env.probe_math(op, M.inputs(op))
    assert np.isfinite(got).all()
    assert (got[:, M.N_OUT.get(op, 1):] == 0.0).all()          # the rest of a row is zero
    ok, msg = M.compare(op, got)
    print(msg)
    assert ok, msg


def test_two_probe_runs_are_bit_identical(env):
    for op in M.OPS:
        a, b = env.probe_math(op, M.inputs(op)), env.probe_math(op, M.inputs(op))
        assert a.tobytes() == b.tobytes(), op


def test_probe_refuses_bad_arguments(env, pkg):
    lib, capi = env.lib, pkg.capi
    src = np.ones((4, capi.AC_PROBE_IN))
    dst = np.full((4, capi.AC_PROBE_OUT), 7.0)
    cases = {
        "unknown op": (env._h, len(capi.AC_PROBE_OPS), 4, src.ctypes.data, dst.ctypes.data),
        "negative op": (env._h, -1, 4, src.ctypes.data, dst.ctypes.data),
        "null input": (env._h, 0, 4, None, dst.ctypes.data),
        "null output": (env._h, 0, 4, src.ctypes.data, None),
        "n = 0": (env._h, 0, 0, src.ctypes.data, dst.ctypes.data),
        "n < 0": (env._h, 0, -4, src.ctypes.data, dst.ctypes.data),
        "n too large": (env._h, 0, capi.AC_PROBE_MAX_ROWS + 1, src.ctypes.data, dst.ctypes.data),
        "null handle": (None, 0, 4, src.ctypes.data, dst.ctypes.data),
    }
    for what, args in cases.items():
        assert lib.ac_probe_math(*args) != 0, what
        assert lib.last_error().startswith("ac_probe_math: "), (what, lib.last_error())
        assert (dst == 7.0).all(), what
    with pytest.raises(RuntimeError, match="ac_probe_math failed: ac_probe_math: unknown op"):
        env.probe_math(len(capi.AC_PROBE_OPS), src)
    assert env.probe_math("fx_rcp", [2.0, 4.0])[:, 0].tolist() == [0.5, 0.25]   # (and a good call still works afterwards)
