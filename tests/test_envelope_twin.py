"""The envelope harness (tests/envelope_util.py) held to account without a GPU: the oracle against a second oracle, teacher-forced, on
the very locations, cells, seeds and bounds that tests/test_gpu_envelope.py sets the device.

control         the oracle against itself: every difference is exactly 0;
fp32 twin       the second oracle starts every step from the state rounded to float32 (entries vx..tank1; the position stays fp64):
                what a correct fp32 implementation may differ by. It must meet every condition the GPU test sets the device; the
                fraction of each bound it uses is printed per location, atmosphere layer and Mach band;
coverage        the oracle's own states reach all three atmosphere layers, Mach < 0.4 and > 1.2, alpha > 25 deg and < -10 deg,
                |beta| > 8 deg, both hemispheres, every longitude quadrant, the afterburner on and off, each for a stated number of
                samples; the steps on which an episode ends (compared on done and reward only) stay under 5 % of all;
planted faults  five faults put into the second oracle's imported state only. The harness must catch each within two steps, in every
                cell group where the fault acts, and nowhere else.
refusal         an initial condition on a pole is refused by config_from_dict and by ac_create."""
import numpy as np
import pytest

import envelope_util as U


@pytest.fixture(scope="module")
def ix(pkg):
    return U.field_index(pkg)


@pytest.fixture(scope="module")
def refs(pkg, oracle):
    return [U.reference(pkg, oracle, i) for i in range(len(U.LOCATIONS))]


def test_control_oracle_against_itself_is_exact(oracle, refs, ix):
    for ref in refs:
        rep = U.compare(ref, U.OracleUnderTest(oracle, ref), ix)
        for q, used in rep.used().items():
            assert used == 0.0, (ref.name, q, used)
        assert not rep.violations


def test_fp32_twin_meets_the_gpu_tests_conditions(oracle, refs, ix):
    tables, worst, force_plain = [], {}, ("", 0.0)
    for ref in refs:
        rep = U.compare(ref, U.OracleUnderTest(oracle, ref, U.fp32_twin), ix)
        tables.append(rep.by_group())
        force_plain = max(force_plain, rep.force_plain, key=lambda t: t[1])
        for q, v in rep.used().items():
            worst[q] = max(worst.get(q, 0.0), v)
    U.print_used("fp32 twin", U.merge_used(tables))
    print("fp32 twin, worst over the envelope:", {q: round(v, 4) for q, v in worst.items()},
          "; most that a force word uses of its bound WITHOUT the dynamic-pressure factor:", force_plain)
    assert force_plain[1] > 1.0         # the twin itself needs envelope_util.Q_REF's widening: rounding the inputs alone exceeds the plain bound
    # rounding the INPUT state moves one step's outputs by a small part of the one-step bounds (observations and rewards: 1e-3 of
    # them); the stored accelerations, differences of forces, carry the most
    assert max(worst.values()) <= 1.0 and worst["obs"] <= 0.05 and worst["rew"] <= 0.05, worst


@pytest.mark.parametrize("task", ["multiplecombat", "scenario_nvn"])
def test_fp32_twin_meets_the_nvn_conditions(pkg, oracle, ix, task):
    worst = {}
    for loc in U.NVN_LOCATIONS:
        ref = U.reference(pkg, oracle, loc, E=6, task=task, per_side=2, per_env=False, chaff_seed=9)
        rep = U.compare(ref, U.OracleUnderTest(oracle, ref, U.fp32_twin), ix, record=False)
        for q, v in rep.used().items():
            worst[q] = max(worst.get(q, 0.0), v)
    print(f"fp32 twin, {task} 2v2, worst over the locations:", {q: round(v, 4) for q, v in worst.items()})
    assert worst["obs"] <= 0.05 and worst["rew"] <= 0.05, worst


# sample counts that the committed grid and seed must reach: about half of what they do reach (printed by the test; 5 136 samples:
# layers 1996 / 1677 / 1393, Mach < 0.4 1014, Mach > 1.2 1535, alpha > 25 deg 173, alpha < -10 deg 122, |beta| > 8 deg 481, northern 3504,
# southern 1529, longitude quadrants 816 / 1064 / 851 / 2335, augmentation on 3681, off 1385; 1.36 % of the steps end an episode)
COVERAGE_FLOOR = {"troposphere": 1000, "isothermal": 800, "upper gradient": 700, "Mach < 0.4": 500, "Mach > 1.2": 750, "alpha > 25 deg": 80,
                  "alpha < -10 deg": 60, "|beta| > 8 deg": 240, "northern": 1700, "southern": 750, "longitude -180..-90": 400,
                  "longitude -90..0": 500, "longitude 0..90": 400, "longitude 90..180": 1100, "augmentation on": 1800, "augmentation off": 700}


def test_coverage_and_skipped_samples(refs):
    cov = U.coverage(refs)
    skipped = U.skipped_fraction(refs)
    total = sum(r.layer.size for r in refs)
    print(f"envelope coverage ({total} samples, {skipped:.2%} of the (env, step) pairs end an episode):", cov)
    print("Mach", round(min(float(r.mach.min()) for r in refs), 2), "..", round(max(float(r.mach.max()) for r in refs), 2),
          "alpha deg", round(min(float(r.alpha_deg.min()) for r in refs), 1), "..", round(max(float(r.alpha_deg.max()) for r in refs), 1))
    for name, floor in COVERAGE_FLOOR.items():
        assert cov[name] >= floor, (name, cov[name], floor)
    assert skipped <= 0.05, skipped
    # altitudes on either side of both layer boundaries are in the set, and the ragged handle too
    assert refs[U.RAGGED].E == 70 and all(r.E == U.ENVS for i, r in enumerate(refs) if i != U.RAGGED)
    # the cells the handles are created with (the device's reset templates: test_reset_matches_oracle_at_every_location) reach every
    # altitude of the grid -- both upper layers, either side of both boundaries -- and every speed
    cells = [(r.cfg.init[a].h_sl_ft, r.cfg.init[a].u_fps) for r in refs for a in range(2)]
    assert {c[0] for c in cells} == set(U.ALTITUDES) and {c[1] for c in cells} == set(U.SPEEDS)
    assert sum(r.layer[0, 0, a] == 1 for r in refs for a in range(2)) >= 4 and sum(r.layer[0, 0, a] == 2 for r in refs for a in range(2)) >= 4
    assert sum(r.mach[0, 0, a] > 1.2 for r in refs for a in range(2)) >= 4


SOUTHERN = [i for i, l in enumerate(U.LOCATIONS) if l[1] < 0]
NORTHERN = [i for i, l in enumerate(U.LOCATIONS) if l[1] > 0.02]
EVERYWHERE = list(range(len(U.LOCATIONS)))


# (fault, locations where it acts, locations where it must change nothing, first step index at which it acts: the stale words need a step before them)
@pytest.mark.parametrize("fault,acts_in,silent_in,begins", [
    (lambda: U.lost_hemisphere, SOUTHERN, NORTHERN, 0),
    (lambda: U.lost_longitude_sign, EVERYWHERE, [], 0),
    (lambda: U.altitude_300ft_off, EVERYWHERE, [], 0),
    (U.StaleAirData, EVERYWHERE, [], 1),
    (lambda: U.v_w_exchanged, EVERYWHERE, [], 0),
], ids=["rz_sign_lost_in_the_south", "ry_sign_flipped", "altitude_300_ft_off", "stale_alpha_and_mach", "v_and_w_exchanged"])
def test_planted_fault_is_caught_within_two_steps(oracle, refs, ix, fault, acts_in, silent_in, begins):
    caught = {}
    for i in acts_in + silent_in:
        ref = refs[i]
        rep = U.compare(ref, U.OracleUnderTest(oracle, ref, fault()), ix, strict=False)
        first = rep.first_violation_step()
        if i in silent_in:
            assert first is None and max(rep.used().values()) == 0.0, (ref.name, rep.violations[:3])     # the fault does not act here: exact
            continue
        assert first is not None and begins <= first <= begins + 1, (ref.name, first)                    # nothing before the fault, and within two steps of it
        # ... and in every atmosphere layer and Mach band that the location's cells reach
        groups = [(nm, ref.layer == j) for j, nm in enumerate(U.LAYERS)] + [(nm, ref.band == j) for j, nm in enumerate(U.MACH_BANDS)]
        for nm, mask in groups:
            two = slice(begins, begins + 2)
            if (mask[two] & ref.live()[two]).any():
                k = rep.first_violation_step(mask)
                assert k is not None and k <= begins + 1, (ref.name, nm, k)
        caught[ref.name] = len({(v[1], v[2]) for v in rep.violations if v[0] <= begins + 1})
    print("aircraft with a violation within two steps, per location:", caught)


@pytest.mark.parametrize("lat", [90.0, -90.0, 89.9999999, 91.0, float("nan")])
def test_initial_condition_on_a_pole_is_refused(pkg, lat):
    """|lat| = 90 is rsqrtf(0) in f16::locate_fast: refused by the YAML mapping and by ac_create (which checks it before it looks for a
    device), never turned into a non-finite state."""
    data = {"task": "singlecombat", "aircraft_configs": {
        "A0100": {"init_state": {"ic_lat_geod_deg": lat}}, "B0100": {"init_state": {"ic_lat_geod_deg": 60.0}}}}
    with pytest.raises(ValueError, match="latitude|finite"):
        pkg.config.config_from_dict(data)
    cfg = pkg.default_config("singlecombat")
    cfg.init[1].lat_geod_deg = lat
    with pytest.raises(RuntimeError, match="latitude|finite"):
        pkg.HipVecEnv(cfg, 2)


@pytest.mark.parametrize("field,value,word", [("h_sl_ft", 120000.0, "altitude"), ("u_fps", float("inf"), "finite"), ("q_rad_sec", float("nan"), "finite")])
def test_other_unrepresentable_initial_conditions_are_refused_by_ac_create(pkg, field, value, word):
    cfg = pkg.default_config("singlecombat")
    setattr(cfg.init[0], field, value)
    with pytest.raises(RuntimeError, match=word):
        pkg.HipVecEnv(cfg, 2)


def test_the_envelope_locations_are_accepted(pkg):
    for loc in U.LOCATIONS:
        cells = [U.draw_cell(np.random.default_rng(1)) for _ in range(2)]
        cfg = U.location_config(pkg, "singlecombat", loc, cells)
        assert abs(cfg.init[1].lat_geod_deg) <= 85.05 and abs(cfg.init[1].lon_deg) < 180.0 and abs(cfg.init[0].lon_deg) < 180.0
