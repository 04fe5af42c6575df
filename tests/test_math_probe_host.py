"""The references, CPU twins and bounds of tests/math_probe_util.py, checked without a GPU: the exact multiply-add, the twins' figures
behind the bounds, the accuracy claims the twins must meet on their own, the references against the oracle's exports, and the comparison
the GPU test uses, fed twins with one planted fault at a time."""
import ctypes as C
import math
import os
import re

import mpmath as mp
import numpy as np
import pytest

import math_probe_util as M

U53 = 2.0 ** -53
TOLERANT_OPS = [op for op in M.OPS if op not in M.EXACT_OPS and op != "tef_kinematic"]


def test_every_probe_op_has_an_input_set_and_the_names_match_the_header():
    import aircombat_selfplay_amd as pkg
    capi = pkg.capi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aircombat.h")).read()
    enum = header[header.index("AC_PROBE_FX_RCP = 0"):header.index("AC_PROBE_NOPS\n")]
    names = [n[len("AC_PROBE_"):].lower() for n in re.findall(r"^\s*(AC_PROBE_\w+)", enum, flags=re.M)]
    assert tuple(names) == tuple(capi.AC_PROBE_OPS) == M.OPS
    assert f"AC_PROBE_IN = {capi.AC_PROBE_IN}, AC_PROBE_OUT = {capi.AC_PROBE_OUT}, AC_PROBE_MAX_ROWS = 1 << 22" in header and capi.AC_PROBE_MAX_ROWS == 1 << 22
    for op in M.OPS:
        X = M.inputs(op)
        assert 19000 <= X.shape[0] <= 70000 and X.shape[1] <= capi.AC_PROBE_IN, (op, X.shape)
        assert np.isfinite(X).all(), op
        assert M.twin(op).shape[1] == M.N_OUT.get(op, 1) <= capi.AC_PROBE_OUT, op
    for op in M.OPS[5:21] + ("missile_height_f",):        # the fp32 ops read (float)in: their sets are float32-exact
        X = M.inputs(op)
        assert (X.astype(np.float32).astype(np.float64) == X).all(), op


def test_the_twins_multiply_add_is_exact():
    """fma64 / fma32 against a * b + c in 400-bit arithmetic rounded once, on random values, on cancelling ones (c = -round(a b)) and on
    sums that fall on a float32 tie of the double-rounding kind."""
    mp.mp.prec = 400
    g = np.random.default_rng(7)
    a, b = g.standard_normal(3000) * 10.0 ** g.uniform(-8, 8, 3000), g.standard_normal(3000) * 10.0 ** g.uniform(-8, 8, 3000)
    c = np.where(g.random(3000) < 0.5, -(a * b), g.standard_normal(3000) * np.abs(a * b) * 10.0 ** g.uniform(-18, 2, 3000))
    got = M.fma64(a, b, c)
    want = np.array([float(mp.mpf(float(x)) * mp.mpf(float(y)) + mp.mpf(float(z))) for x, y, z in zip(a, b, c)])
    assert (got == want).all()
    a32, b32, c32 = (v.astype(np.float32) for v in (a, b, c))      # (1e-24 <= |a b| <= 1e18 or so: no float32 overflow or underflow)
    a32 = np.concatenate([a32, np.float32([1.0 + 2.0 ** -12, 1.0 + 2.0 ** -23])])
    b32 = np.concatenate([b32, np.float32([1.0 + 2.0 ** -12, 1.0 - 2.0 ** -24])])
    c32 = np.concatenate([c32, np.float32([2.0 ** -60, 2.0 ** -70])])      # (exact product on a tie, pushed off it by a tiny addend)
    got = M.fma32(a32, b32, c32)
    exact = [mp.mpf(float(x)) * mp.mpf(float(y)) + mp.mpf(float(z)) for x, y, z in zip(a32, b32, c32)]
    mp.mp.prec = 24                                                  # (unary plus rounds to the working precision: one rounding, to float32's)
    want = np.array([float(+v) for v in exact], dtype=np.float32)
    assert (got == want).all()


@pytest.mark.parametrize("op", TOLERANT_OPS)
def test_twin_figure_in_the_table_is_reproduced(op):
    """B = 2 x TWIN + A: the table's copy of the twin's worst figure is what the twin gives on the op's input set (within 5 %)."""
    fig = M.figures(op, M.twin(op)).max(axis=0)
    tab = np.asarray(M.TWIN[op])
    assert fig.shape == tab.shape == np.asarray(M.ALLOWANCE[op]).shape
    print(op, "twin", fig, "allowance", M.ALLOWANCE[op], "bound", M.bound(op))
    assert (np.abs(fig - tab) <= 0.05 * tab).all(), (op, fig, tab)


@pytest.mark.parametrize("op", M.OPS)
def test_the_clean_twin_passes_the_gpu_tests_comparison(op):
    ok, msg = M.compare(op, M.twin(op))
    assert ok, msg


def test_fx_twins_meet_the_headers_claim():
    """csrc/fp64_fast.hpp: rcp, rsqrt, sqrt, sqrt_both within 4 x 2^-53 relative; sincos within 2 x 2^-53 absolute and 4 x 2^-53 relative
    over |x| <= 8 pi (with the 1/16! cosine term: without it 9.7 and 13.7, see test_the_comparison_bites)."""
    for op in ("fx_rcp", "fx_rsqrt", "fx_sqrt", "fx_sqrt_both"):
        fig = M.figures(op, M.twin(op)).max(axis=0) / U53
        print(op, fig)
        assert (fig <= 4.0).all(), (op, fig)
    assert M.twin("fx_sqrt")[M.inputs("fx_sqrt")[:, 0] == 0.0, 0].tolist() == [0.0]
    fig = M.figures("fx_sincos", M.twin("fx_sincos")).max(axis=0) / U53
    print("fx_sincos abs, rel", fig)
    assert (fig[:2] <= 2.0).all() and (fig[2:] <= 4.0).all(), fig
    old = M.figures("fx_sincos", M.twin("fx_sincos", fault="no_16")).max(axis=0) / U53
    print("fx_sincos without the 1/16! term", old)
    assert old[1] > 8.0 and old[2:].max() > 10.0


def test_geodesy_twins_meet_their_claims():
    """neu_height64 within 1 mm and missile_height within the figures of its comment, over the +-60 km box, u in [0, 20 km], about the
    shipped centre: 4.1 cm over the box, 9.5 mm over the +-40 km box, 3.5 mm within a 40 km radius. (4 cm over the +-60 km box does not
    hold: the local-curvature form is 40.2 mm off at the (+-60, +-60) km corners at ground level, 39.8 mm there at 20 km. The error is
    the formula's, smooth and largest at the box's corners, which the input set holds exactly; 4.1 cm is that corner value rounded up.)"""
    assert M.figures("neu_height64", M.twin("neu_height64")).max() <= 1e-3
    X = M.inputs("missile_height_d")
    err = M.figures("missile_height_d", M.twin("missile_height_d"))[:, 0]
    errf = M.figures("missile_height_f", M.twin("missile_height_f"))[:, 0]
    radius = np.hypot(X[:, 0], X[:, 1])
    print("missile_height fp64: box", err.max(), "radius 40 km", err[radius <= 40e3].max(), "box 40 km", err[(np.abs(X[:, :2]) <= 40e3).all(axis=1)].max(),
          "fp32: box", errf.max())
    assert err.max() <= 0.041 and errf.max() <= 0.041
    assert err[radius <= 40e3].max() <= 0.0035 + 1e-5
    assert err[(np.abs(X[:, :2]) <= 40e3).all(axis=1)].max() <= 0.0095


def test_locate_fast_twin_stays_within_its_fp32_budget_of_locate():
    """The fp32 part of locate_fast's altitude, as f16_device.hpp gives it. On paper, for altitudes up to 80 000 ft:
    (float)(rad - b) is up to 150 160 ft, half an ulp there 2^-7 = 0.0078 ft; b x ser is up to 70 160 ft and carries five relative
    roundings of 2^-24 (the fp32 constant e2, cos^2, x, the last fma of the series and its product): 5 x 0.0042 = 0.021 ft; the final
    rounding at up to 80 000 ft 0.0039 ft; the series' truncation 7e-5 ft: 0.033 ft in all. The twin stays within that of locate (the
    fp64 form) and of the reference at every latitude and longitude. (0.01 ft does not hold: the twin differs from locate by 0.016 ft,
    two ulps of the fp32 pieces between 65 536 and 131 072 ft, at every altitude from 0 to 80 000 ft.)"""
    X = M.inputs("locate")
    fast, full = M.twin("locate_fast", X)[:, 0], M.twin("locate")[:, 0]
    ref = M.reference("locate")[0][:, 0]
    print("locate_fast - locate", np.abs(fast - full).max(), "locate_fast - reference", np.abs(fast - ref).max(), "locate - reference", np.abs(full - ref).max())
    assert np.abs(fast - full).max() <= 0.033 and np.abs(fast - ref).max() <= 0.033


def test_references_equal_the_oracles_exports(oracle):
    """The restated formulas against the oracle's own: the atmosphere and the kinematic to 1e-12 (relative, absolute), the ellipsoidal
    height to 1e-12 of the 6.4e6 m coordinates it is a difference of."""
    L = oracle.lib()
    out = [C.c_double() for _ in range(5)]
    h = M.inputs("atmosphere")[::97, 0]
    ref = M.ref_atmosphere(h)
    for hi, row in zip(h, ref):
        L.f16_atmosphere(float(hi), *[C.byref(o) for o in out])
        got = np.array([o.value for o in out[:4]])
        assert (np.abs(got - row) <= 1e-12 * np.abs(row)).all(), (hi, got, row)
    det, tt = (C.c_double * 3)(-1.0, 0.0, 1.0), (C.c_double * 3)(3.0, 0.0, 3.0)
    L.f16_kinemat.restype = C.c_double
    X = M.inputs("tef_kinematic")
    for o, i in np.concatenate([X[::53], X[-6:]]):
        want = L.f16_kinemat(float(o), float(i), det, tt, 3, 1.0 / 120.0)
        assert abs(M.ref_kinemat(float(o), float(i))[0] - want) <= 1e-12, (o, i)
    lla = (C.c_double * 3)()
    X = M.inputs("neu_height64")
    sel = np.concatenate([np.arange(0, X.shape[0], 101), np.arange(X.shape[0] - 27, X.shape[0])])
    ref = M.ref_neu_height(X[sel, 0], X[sel, 1], X[sel, 2])
    hi, lo = M.reference("neu_height64")
    for k, (n, e, u) in zip(sel, X[sel]):
        L.or_neu2lla(float(n), float(e), float(u), M.CENTER[1], M.CENTER[0], M.CENTER[2], lla)
        assert abs(lla[2] - ref[list(sel).index(k)]) <= 1e-12 * M.WGS_A, (n, e, u)
        assert abs((lla[2] - hi[k, 0]) - lo[k, 0]) <= 1e-12 * M.WGS_A, (n, e, u)


def test_wrap_twins_follow_utils_py_and_the_pitot_inverse_inverts():
    for op, per in (("in_range_deg", 360.0), ("in_range_rad", 2 * math.pi)):
        a = M.inputs(op)[:, 0]
        d = np.abs(M.twin(op)[:, 0] - M.reference(op)[0][:, 0])
        d = np.minimum(d, np.abs(d - per))                  # (-half a period and +half a period are one direction)
        # each whole period taken off carries the float32 period's distance from the true one; then three float32 roundings below a period
        tol = np.abs(a) / per * abs(float(np.float32(per)) - per) + 3 * per * 2.0 ** -24
        assert (d <= tol).all(), (op, a[np.argmax(d - tol)], d.max())
    # vcas's input set is pitot's output: the 10-step inverse brings the Mach number back, exactly below Mach 1 and, above it, to the
    # 0.417^10 = 1.6e-4 of the first guess's error that ten passes of the contraction leave
    g = np.random.default_rng(3)
    m = np.concatenate([g.uniform(0.1, 2.2, 2000), [0.999999, 1.000001]])
    back = M.ref_mach_from_qc(M.ref_pitot(m, M.ATM_PSL))
    assert np.abs(back - m)[m < 1.0].max() <= 1e-12
    assert (np.abs(back - m)[m >= 1.0] <= 1.6e-4 * m[m >= 1.0]).all()


def test_tef_kinematic_leaves_out_at_most_one_percent_and_holds_the_detents():
    keep = M.tef_keep()
    assert keep.mean() >= 0.99
    X = M.inputs("tef_kinematic")
    assert X[-6:-3].tolist() == [[0.0, float(np.float32(-0.1))], [float(np.float32(-0.1)), float(np.float32(0.9))], [0.0, 1.0]] and keep[-6:].all()
    ref = M.reference("tef_kinematic")[0][-6:-3, 0]
    # (into the zero-time segment: jump; out of it from below: the segment the output starts in is the zero-time one, jump; from 0 up: walk)
    assert np.allclose(ref, [float(np.float32(-0.1)), float(np.float32(0.9)), 1.0 / 360.0], rtol=0, atol=1e-15)


def _quarter_turns(X):
    return np.rint(X[:, 0] * 0.63661977236758134308)


FAULTS = [
    # op, fault, what a failing row must look like (a predicate over the op's input rows)
    ("fx_sincos", "no_16", lambda X: np.abs(X[:, 0] - np.rint(X[:, 0] / (math.pi / 2)) * (math.pi / 2)) > 0.5),     # the far end of the octant
    ("fx_sincos", "coef", lambda X: np.abs(X[:, 0] - _quarter_turns(X) * (math.pi / 2)) > 1e-3),
    ("fx_sincos", "quadrant", lambda X: np.isin(_quarter_turns(X).astype(np.int64) & 3, (1, 3))),
    ("atan2_fast", "drop", lambda X: np.minimum(np.abs(X[:, 0]), np.abs(X[:, 1])) > 0.3 * np.maximum(np.abs(X[:, 0]), np.abs(X[:, 1]))),
    ("atan2_fast", "coef", lambda X: np.minimum(np.abs(X[:, 0]), np.abs(X[:, 1])) > 0.1 * np.maximum(np.abs(X[:, 0]), np.abs(X[:, 1]))),
    ("atan2_fast", "quadrant", lambda X: X[:, 1] != 0),
    ("atmosphere", "coef", lambda X: X[:, 0] * M.ATM_RE / (M.ATM_RE + X[:, 0]) < M.ATM_H[1]),
    ("posture_fn", "coef", lambda X: X[:, 2] >= 5.0),
    ("missile_height_d", "drop", lambda X: np.abs(X[:, 1]) > 100.0),
    ("tef_kinematic", "lt", lambda X: (X[:, 0] == 0.0) & (X[:, 1] > 0.0)),
    ("in_range_deg", "ge", lambda X: np.fmod(np.abs(X[:, 0]), 360.0) == 180.0),
]


@pytest.mark.parametrize("op,fault", [(op, f) for op, f, _ in FAULTS])
def test_the_comparison_bites(op, fault):
    """The GPU test's comparison fed a twin with one planted fault -- a dropped last polynomial term (the parent's sincos without 1/16!
    among them), a coefficient 1e-3 off, a swapped quadrant sign, < for <= at a boundary -- fails, and fails only where the fault acts.
    (The atmosphere's layers join continuously, so < for <= at a layer boundary changes no value there; the boundary faults are planted
    where the two sides differ: the flap kinematic's detent at 0 and the wrap at half a period.)"""
    where = next(w for o, f, w in FAULTS if (o, f) == (op, fault))
    got = M.twin(op, fault=fault)
    ok, msg = M.compare(op, got)
    print(msg)
    assert not ok, msg
    bad = M.mismatches(op, got) if op in M.EXACT_OPS else (M.ratios(op, got) > 1.0).any(axis=1)
    assert bad.any() and where(M.inputs(op))[bad].all(), (op, fault, M.inputs(op)[bad & ~where(M.inputs(op))][:5])
