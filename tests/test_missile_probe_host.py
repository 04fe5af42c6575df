"""The cases, reference, twins and bounds of tests/missile_probe_util.py, checked without a GPU: what the cases reach (from the oracle's own
runs), the cap on rows left out of the discrete comparison, the restated reference against the oracle and the fixture, the twins' figures
behind the bounds, the comparison the GPU test uses fed twins with one planted fault at a time, and the probe's refusals that return
before any device call."""
import math
import os

import numpy as np
import pytest

import missile_probe_util as M

ALL = [(name, form) for name in M.GROUPS for form, _ in M.GROUPS[name][2]]


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


def test_header_capi_and_util_agree():
    import aircombat_selfplay_amd as pkg
    capi = pkg.capi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aircombat.h")).read()
    assert (f"AC_PROBE_MSL_IN = {capi.AC_PROBE_MSL_IN}, AC_PROBE_MSL_TGT = {capi.AC_PROBE_MSL_TGT}, AC_PROBE_MSL_OUT = {capi.AC_PROBE_MSL_OUT}, "
            f"AC_PROBE_MSL_MAX_ROWS = {capi.AC_PROBE_MSL_MAX_ROWS}, AC_PROBE_MSL_MAX_TICKS = {capi.AC_PROBE_MSL_MAX_TICKS}") in header
    assert "AC_PROBE_MSL_MAX_CELLS = 1 << 19" in header and capi.AC_PROBE_MSL_MAX_CELLS == 1 << 19
    assert f"AC_PROBE_MSL_FP32 = {M.FP32}, AC_PROBE_MSL_FP64 = {M.FP64}" in header and f"AC_PROBE_MSL_AIM9L = {M.AIM9L}, AC_PROBE_MSL_AIM120B = {M.AIM120B}" in header
    assert M.N_OUT == capi.AC_PROBE_MSL_OUT
    for name in M.GROUPS:
        launch, target, _, combos = M.group(name)
        ticks, n = target.shape[:2]
        assert n <= capi.AC_PROBE_MSL_MAX_ROWS and ticks <= capi.AC_PROBE_MSL_MAX_TICKS and n * ticks <= capi.AC_PROBE_MSL_MAX_CELLS, name
        assert launch.shape == (n, capi.AC_PROBE_MSL_IN) and target.shape[2] == capi.AC_PROBE_MSL_TGT
        assert set(combos) <= set(M.PRODUCTION)
    assert {c for name in M.GROUPS for c in M.GROUPS[name][2]} == set(M.PRODUCTION)


def test_tick_counts_follow_the_running_sum():
    """Burn-out and time-out as tick counts, from the float64 running sum of 1/60 the reference keeps (aircombat.hip states 84 and 180
    additions against 1.4 and 3.0)."""
    assert M.K_BURNOUT == {M.AIM9L: 181, M.AIM120B: 84}
    assert M.K_TIMEOUT == {M.AIM9L: 3601, M.AIM120B: 1634}


def test_the_cases_reach_what_they_are_meant_to():
    cov = M.coverage()
    every = {"hit", "timeout", "v_min", "recede", "target_death"}
    assert cov["causes"][M.AIM9L] == every and cov["causes"][M.AIM120B] == every      # (both k_timeout values among them)
    assert cov["burnout"] == {M.AIM9L: {M.K_BURNOUT[M.AIM9L]}, M.AIM120B: {M.K_BURNOUT[M.AIM120B]}}
    assert cov["fallback_rows"] >= 20            # a per-tick |d psi| or |d theta| above 0.05: the full sincos path of the fp64 overload
    assert cov["over_top_hits"] >= 10            # stored |theta| past pi / 2 in flight, and the oracle ends the row in HIT
    assert cov["saturated"] >= 10                # MISS by 300 receding ticks in a row, the oracle's count running on past 300
    assert min(cov["altitudes"]) == 1000.0 and max(cov["altitudes"]) == 18000.0
    assert len(cov["quadrants"]) == 4 and cov["steep_dives"] >= 20 and cov["dies_in_flight"] >= 10
    assert cov["centers"] == set(M.CENTERS.values()) and len(cov["centers"]) == 4
    # the four over-the-top starts are rows of the AIM-120B grid, the first of them a HIT at tick 166 in the oracle
    launch, target, _, _ = M.group("over_top_120b")
    facts = M.facts(M.oracle_run("over_top_120b"), launch, M.AIM120B)
    for r, (north, up, pitch, tvn) in enumerate(M.OVER_THE_TOP_STARTS):
        assert launch[r, 6] == pitch and target[0, r, 3] == pytest.approx(tvn) and target[0, r, 2] == 6000.0 + up
        assert abs(target[0, r, 0] - (north + tvn / 60.0)) < 1e-9
    assert facts[0]["cause"] == "hit" and facts[0]["end"] + 1 == 166 and 1.67 < facts[0]["max_theta"] < 1.68
    assert all(f["max_theta"] > math.pi / 2 for f in facts[:4])
    assert max(max(f["max_dpsi"], f["max_dtheta"]) for f in facts) > 0.08           # (the fp64 overload's full-sincos path starts at 0.05)
    # the fixture's seven fly-outs
    assert M.group("golden_9l")[0].shape[0] + M.group("golden_120b")[0].shape[0] == 7


@pytest.mark.parametrize("name,form", ALL)
def test_the_oracle_stays_inside_the_cap_on_undecided_rows(name, form):
    """At most 2 % of a group's rows have their discrete comparison cut short, in every group and form, the fixture's fly-outs and the
    four named over-the-top starts included; and what the plan leaves out elsewhere is a small part of the facts."""
    pl = M.plan(name, form)
    cut = pl["cut"]
    print(f"{name} form {form}: {int(cut.sum())} of {cut.size} rows cut short, {int(pl['windowed'].sum())} with an ending window; compared: "
          f"status {pl['status'].mean():.3f}, moved {pl['moved'].mean():.3f}, count {pl['rec'].mean():.3f}, mass {pl['mass'].mean():.3f} of all ticks")
    assert cut.sum() <= M.EXCLUDE_CAP * cut.size, (name, form, np.nonzero(cut)[0])
    assert not cut[:M.NAMED_STARTS.get(name, 0)].any()
    assert pl["status"].mean() >= 0.98 and pl["status"][0].all()


def _close(a, b, rtol, atol):
    with np.errstate(invalid="ignore"):
        return (np.abs(a - b) <= atol + rtol * np.abs(b)) | ((a == b))


def test_restated_reference_matches_the_fixture_rows():
    """fly("ref") on the fixture's launches against the fixture's own rows, at the tolerances of test_missile_flyouts."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "missile.npz"))
    for model in (M.AIM9L, M.AIM120B):
        launch, target, ids = M._golden_group(model)
        out = M.fly("ref", model, launch, target)
        for r, c in enumerate(ids):
            rows = g[f"c{c}_rows"]
            got = out[:len(rows), r]
            assert (got[:, M.O_STATUS] == rows[:, 2]).all(), c
            assert _close(got[:, 1:4], rows[:, 9:12], 1e-9, 1e-6).all(), c
            assert _close(got[:, 4:7], rows[:, 12:15], 1e-9, 1e-7).all(), c
            assert _close(got[:, 7:9], rows[:, 15:17], 1e-9, 1e-9).all(), c
            assert _close(got[:, 9:11], rows[:, 17:19], 1e-9, 1e-6).all(), c


@pytest.mark.parametrize("name", ["golden_9l", "golden_120b", "endings_120b", "centre_equator", "centre_arctic", "centre_antarctic"])
def test_restated_reference_matches_the_oracle(name):
    """... and against the oracle at the same tolerances, at every centre: the discrete facts at every tick, the continuous fields at
    every tick of the fixture's fly-outs and, elsewhere, while the missile closes (after a pass a fly-out magnifies the last bit)."""
    launch, target, center, combos = M.group(name)
    ora = M.oracle_run(name)
    out = M.fly("ref", combos[0][1], launch, target, center)
    for col in (M.O_STATUS, M.O_REC, M.O_MOVED):
        assert (out[:, :, col] == ora[:, :, col]).all(), (name, col)
    if name not in M.FIXTURE_GROUPS:
        win = M.window(name)[:, :, None]
        out, ora = np.where(win, out, 0.0), np.where(win, ora, 0.0)
    assert _close(out[:, :, 1:4], ora[:, :, 1:4], 1e-9, 1e-6).all()
    assert _close(out[:, :, 4:7], ora[:, :, 4:7], 1e-9, 1e-7).all()
    assert _close(out[:, :, 7:9], ora[:, :, 7:9], 1e-9, 1e-9).all()
    assert _close(out[:, :, 9:11], ora[:, :, 9:11], 1e-9, 1e-6).all()
    assert _close(out[:, :, 11:14], ora[:, :, 11:14], 1e-9, 1e-7).all()


def test_restated_reference_follows_the_oracle_over_the_top():
    """Past pi / 2 the fly-outs are ill-conditioned (ny / cos theta); the restatement still follows the oracle to millimetres while the
    missile closes, and ends every row the same way at the same tick."""
    launch, target, center, _ = M.group("over_top_120b")
    ora = M.oracle_run("over_top_120b")
    out = M.fly("ref", M.AIM120B, launch, target, center)
    win = M.window("over_top_120b")
    assert np.where(win[:, :, None], np.abs(out[:, :, 1:4] - ora[:, :, 1:4]), 0.0).max() < 3e-3
    assert (out[:, :, M.O_STATUS] == ora[:, :, M.O_STATUS]).all()


@pytest.mark.parametrize("name,form", ALL)
def test_twin_figure_in_the_table_is_reproduced(name, form):
    """B = 2 x |twin - oracle| + A: the table's copy of the twin's worst deviation inside the comparison window is what the twin gives
    (within 5 %), and the twin itself passes the comparison it underlies."""
    fig = M.twin_figures(name, form)
    print(name, form, tuple(float(f"{x:.4g}") for x in fig))
    want = M.TWIN[(name, form)]
    for got, w in zip(fig, want):
        assert abs(got - w) <= 0.05 * w, (name, form, fig, want)
    ok, worst, msg = M.compare(name, form, _as_device(M.twin_run(name, form)[0], form))
    assert ok and max(worst.values()) <= 0.5, msg


def _as_device(out, form):
    out = out.copy()
    if form == M.FP32:
        out[:, :, M.O_MOVED] = -1.0
    return out


def _faulted(name, form, fault):
    launch, target, center, combos = M.group(name)
    model = [m for f, m in combos if f == form][0]
    return _as_device(M.fly("twin32" if form == M.FP32 else "twin64", model, launch, target, center, fault=fault), form)


# fault -> (group, form, what the comparison must name)
PLANTED = {
    "abs_cos": ("over_top_120b", M.FP64, ("status", "pos")),
    "burnout_late": ("endings_120b", M.FP64, ("burn-out",)),
    "timeout_ge": ("endings_9l", M.FP64, ("status",)),
    "recede_noreset": ("envelope_120b", M.FP64, ("recede",)),
    "recede_nosat": ("endings_120b", M.FP64, ("recede",)),
    "guidance_f32": ("envelope_120b", M.FP64, ("pos",)),
    "height_off": ("envelope_120b", M.FP64, ("vel",)),
    "dprev_frozen": ("endings_120b", M.FP64, ("dprev",)),
    "tvz_negated": ("envelope_120b", M.FP64, ("pos",)),
}


@pytest.mark.parametrize("fault", sorted(PLANTED))
def test_comparison_fails_for_a_planted_fault(fault):
    name, form, named = PLANTED[fault]
    ok, worst, msg = M.compare(name, form, _faulted(name, form, fault))
    print(msg)
    assert not ok, msg
    for what in named:
        assert what + ":" in msg, (what, msg)


def test_fp32_near_the_vertical_two_roundings_fly_apart_and_the_window_ends_before():
    """Why the fp32 continuous comparison stops where the stored pitch comes within COS_MIN_F32 of the vertical: a second correctly rounded
    fp32 arithmetic, an ulp off in the speed's root and the rebuilt sines and cosines at every tick, stays within 2 cm of the twin inside
    that window and flies more than 10 m from it beyond, in the over-the-top grid. Jittered twins that the bound has not seen pass the
    whole comparison, discrete facts at every tick included."""
    launch, target, center, _ = M.group("over_top_9l")
    tw = M.twin_run("over_top_9l", M.FP32)[0]
    other = M.fly("twin32", M.AIM9L, launch, target, center, jitter=7)
    inside = M.window("over_top_9l", M.FP32)
    beyond = M.window("over_top_9l", M.FP64) & ~inside
    apart = np.abs(tw[:, :, 1:4] - other[:, :, 1:4])
    assert np.where(inside[:, :, None], apart, 0.0).max() < 0.02 and np.where(beyond[:, :, None], apart, 0.0).max() > 10.0
    assert inside.sum() > 0.25 * M.window("over_top_9l", M.FP64).sum()         # (the window keeps over a quarter of the grid's closing ticks)
    for name in ("over_top_9l", "envelope_9l"):
        launch, target, center, _ = M.group(name)
        for seed in (7, 8):
            ok, _, msg = M.compare(name, M.FP32, _as_device(M.fly("twin32", M.AIM9L, launch, target, center, jitter=seed), M.FP32))
            assert ok, msg


def test_a_continuous_fault_shows_in_fp32():
    """The fp32 bound bites as well: the density taken 100 m off moves the speed beyond it."""
    ok, _, msg = M.compare("envelope_9l", M.FP32, _faulted("envelope_9l", M.FP32, "height_off"))
    print(msg)
    assert not ok and "vel:" in msg, msg


def test_timeout_fault_also_shows_in_fp32():
    ok, _, msg = M.compare("endings_9l", M.FP32, _faulted("endings_9l", M.FP32, "timeout_ge"))
    assert not ok and "status:" in msg, msg


def test_over_the_top_fault_fails_on_the_over_the_top_rows_only():
    """The velocity-ratio shortcut (cos theta taken as hxy / v >= 0) turns the oracle's HITs past pi / 2 into misses and passes
    everywhere the stored pitch stays inside [-pi / 2, pi / 2]."""
    got = _faulted("over_top_120b", M.FP64, "abs_cos")
    ora = M.oracle_run("over_top_120b")
    launch = M.group("over_top_120b")[0]
    facts = M.facts(ora, launch, M.AIM120B)
    over = np.array([f["max_theta"] > math.pi / 2 for f in facts])
    differs = (got[:, :, M.O_STATUS] != ora[:, :, M.O_STATUS]).any(axis=0)
    assert differs[0] and got[-1, 0, M.O_STATUS] == M.MISS and ora[165, 0, M.O_STATUS] == M.HIT
    assert differs[over].sum() >= 8 and not differs[~over].any()
    ok, _, msg = M.compare("envelope_120b", M.FP64, _faulted("envelope_120b", M.FP64, "abs_cos"))
    assert ok, msg                                # (a benign envelope shows nothing)


def test_gain_without_its_max_cannot_show():
    """K = max(K0 (t_max - t) / t_max, 0) only goes negative once t > t_max, and at that tick run() has already declared the missile MISS
    (:528) without calling _state_trans: the demands that K scales are never used. The planted fault is therefore invisible in every
    output -- the twin without the max is bit for bit the twin -- and is kept here so that a change of the time-out rule shows."""
    for name, form in (("endings_9l", M.FP64), ("endings_120b", M.FP64)):
        assert _faulted(name, form, "gain_no_max").tobytes() == _as_device(M.twin_run(name, form)[0], form).tobytes()


def test_probe_refusals_that_return_before_a_device_call():
    """Every argument check comes before the handle is looked at, so a null handle shows them all without a GPU."""
    import aircombat_selfplay_amd as pkg
    capi = pkg.capi
    lib = pkg.load_library()
    src = np.zeros((4, capi.AC_PROBE_MSL_IN))
    tgt = np.zeros((8, 4, capi.AC_PROBE_MSL_TGT))
    dst = np.full((8, 4, capi.AC_PROBE_MSL_OUT), 7.0)
    good = [None, M.FP64, M.AIM120B, 4, 8, src.ctypes.data, tgt.ctypes.data, dst.ctypes.data]
    expect = {"unknown form": "unknown form", "negative form": "unknown form", "unknown model": "unknown model",
              "fp32 with the AIM-120B set": "no step kernel flies", "n = 0": "n out of range", "n < 0": "n out of range", "n too large": "n out of range",
              "ticks = 0": "ticks out of range", "ticks too large": "ticks out of range", "null launch": "null argument", "null target": "null argument",
              "null output": "null argument", "null handle": "null handle"}
    for what, i, bad in M.REFUSALS(capi):
        args = list(good)
        args[i] = bad
        assert lib.ac_probe_missile(*args) != 0, what
        assert lib.last_error().startswith("ac_probe_missile: ") and expect[what] in lib.last_error(), (what, lib.last_error())
        assert (dst == 7.0).all(), what
    args = list(good)
    args[3], args[4] = capi.AC_PROBE_MSL_MAX_ROWS, capi.AC_PROBE_MSL_MAX_TICKS
    assert lib.ac_probe_missile(*args) != 0 and "n * ticks out of range" in lib.last_error()
