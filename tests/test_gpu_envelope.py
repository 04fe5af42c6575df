"""The device step held to the oracle away from the one spawn point: tests/envelope_util.py's locations and cells on the device.

reset                 every location's handle is created with an envelope initial condition of its own (altitude and speed walk through
                      the grids: every layer, sub- and supersonic; body v / w and body rates non-zero) and reset() is compared with the
                      oracle's: observations and every named state word, with the per-field bounds of
                      test_gpu_parity.py::test_reset_matches_oracle. The device's initial-condition pass away from the default.
teacher-forced        singlecombat in both kernel forms (AIRCOMBAT_SPLIT = 1 three-wave, 0 one-wave), every location, 16 envs each (70 at
                      one: a ragged last workgroup), every env its own cell: observations (parity_util.obs_bounds, scale 1), rewards
                      (RewardBound, scale 1), `done` equal, the whole stored record of every aircraft with the bounds of
                      test_singlecombat_kernel_forms_teacher_forced (the force words x max(1, qbar / 405): envelope_util.Q_FIELDS),
                      and the pose ac_get_entity reports with the first step of the free-flight envelope (envelope_util.pose_fraction).
other families        multiplecombat 2v2 and scenario_nvn 2v2 (pair form, weapon bits 0) through HipShareVecEnv, and heading, at a
                      southern, a western, an equatorial and a far-northern location: each family reduces geodetic -> NEU itself
                      (observations, rewards, `done`, reported pose).
Every test prints the worst fraction of each bound used per location, atmosphere layer and Mach band. tests/test_envelope_twin.py holds
the harness to account on the CPU (control, fp32 twin, coverage, planted faults) with these very cells and seeds.

Measured on the MI355X (DESIGN.md section 8 has the table per group): the device holds every bound in every cell in both forms; worst
fractions used: observation 0.26, reward 0.012, reported pose 0.16, record 0.75 (`pin_y`, with the dynamic-pressure factor; 2.5 / 2.8 of
its plain bound, where the CPU's fp32 twin uses 1.88), reset observation 0.010, reset state 0.35."""
import numpy as np
import pytest

import envelope_util as U
from test_gpu_parity import HEADING_OBS_X, HEADING_REW_X, VECTOR_FIELDS, obs_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ix(pkg):
    return U.field_index(pkg)


@pytest.mark.parametrize("loc", range(len(U.LOCATIONS)), ids=U.LOCATION_IDS)
def test_reset_matches_oracle_at_every_location(pkg, oracle, loc):
    ref = U.reference(pkg, oracle, loc)
    env = pkg.HipVecEnv(ref.cfg, 3)
    obs, robs = env.reset(), ref.reset_obs[0]                       # env 0 of the reference flies the handle's own cells
    names = env.lib.state_field_names()
    tol, free = U.obs_bounds(robs, 1.0)
    used = {"obs": float(np.where(free, 0.0, np.abs(obs - robs[None]) / tol[None]).max())}
    bad = []
    for e in (0, 2):
        for agent in range(2):
            g, o = env.get_state(e, agent), ref.reset_state[0, agent]
            for k, nm in enumerate(names):
                if not nm or nm.startswith("x_"):
                    continue
                scale = abs(o[k])
                for grp in VECTOR_FIELDS:          # components of one vector share the vector's scale
                    if nm in grp:
                        scale = float(np.sqrt(sum(o[names.index(c)] ** 2 for c in grp)))
                tol_k = 0.05 if nm in ("rx", "ry", "rz") else 2e-5 * max(1.0, scale) + 1e-6
                if nm in ("hv1x", "hv1y", "hv1z", "hv2x", "hv2y", "hv2z", "vx", "vy", "vz"):
                    tol_k = 2e-4
                frac = abs(g[k] - o[k]) / tol_k
                used[nm] = max(used.get(nm, 0.0), frac)
                if not frac <= 1.0:
                    bad.append((e, agent, nm, g[k], o[k], tol_k))
    env.close()
    cells = [(round(ref.cfg.init[a].h_sl_ft), ref.cfg.init[a].u_fps) for a in range(2)]
    top = sorted(used.items(), key=lambda t: -t[1])[:6]
    print(f"reset at {ref.name}, cells (ft, ft/s) {cells}: observation bound used {used['obs']:.3f}; most used state bounds",
          {k: round(v, 3) for k, v in top})
    assert used["obs"] <= 1.0 and not bad, (ref.name, cells, used["obs"], bad[:8])


@pytest.mark.parametrize("three_waves", ["1", "0"], ids=["three_wave", "one_wave"])
def test_singlecombat_teacher_forced_across_the_envelope(pkg, oracle, ix, monkeypatch, three_waves):
    monkeypatch.setenv("AIRCOMBAT_SPLIT", three_waves)
    tables, violations, worst_field, force_plain = [], [], {}, ("", 0.0)
    for loc in range(len(U.LOCATIONS)):
        ref = U.reference(pkg, oracle, loc)
        side = U.DeviceSide(pkg, ref, ix)
        side.reset()
        rep = U.compare(ref, side, ix, strict=False)
        side.close()
        tables.append(rep.by_group())
        violations += [(ref.name,) + v + (U.describe(ref, [v])[0],) for v in rep.violations]
        force_plain = max(force_plain, rep.force_plain, key=lambda t: t[1])
        for cls, (f, v) in rep.worst_field.items():
            if v > worst_field.get(cls, ("", -1.0))[1]:
                worst_field[cls] = (f, round(v, 3))
    U.print_used(f"singlecombat, AIRCOMBAT_SPLIT={three_waves}", U.merge_used(tables))
    print("most used record bound per class:", worst_field, "; most that a force word uses of its bound WITHOUT the dynamic-pressure factor (not asserted):", force_plain)
    assert not violations, (len(violations), violations[:12])


@pytest.mark.parametrize("task,fdm_only", [("multiplecombat", False), ("scenario_nvn", True)])
def test_nvn_families_at_other_locations(pkg, oracle, ix, task, fdm_only):
    tables, violations = [], []
    for loc in U.NVN_LOCATIONS:
        ref = U.reference(pkg, oracle, loc, E=6, task=task, per_side=2, per_env=False, chaff_seed=9)
        side = U.DeviceSide(pkg, ref, ix, share=True, fdm_only=fdm_only, seed=9)
        obs = side.reset()
        tol, free = U.obs_bounds(ref.reset_obs, 1.0)
        bad = (np.abs(obs - ref.reset_obs) > tol) & ~free
        assert not bad.any(), (task, ref.name, "reset", np.argwhere(bad)[:4].tolist(), obs[bad][:4], ref.reset_obs[bad][:4])
        rep = U.compare(ref, side, ix, record=False, strict=False)
        side.close()
        tables.append(rep.by_group())
        violations += [(ref.name,) + v + (U.describe(ref, [v])[0],) for v in rep.violations]
    U.print_used(f"{task} 2v2", U.merge_used(tables))
    assert not violations, (len(violations), violations[:12])


def test_heading_task_at_other_locations(pkg, oracle):
    """The heading env's own geodetic reduction and its reset draws (altitude 14 000 - 30 000 ft, 400 - 1 200 ft/s from numpy's stream)
    at other latitudes and longitudes, with body v / w and body rates in the initial condition. Flight-model fields re-synchronised
    each step, the task's bookkeeping its own; the heading task's existing multiples of the one-step bounds."""
    E, seed, steps = 6, 11, 40
    used = {}
    for loc in U.NVN_LOCATIONS:
        name, lat, lon = U.LOCATIONS[loc][:3]
        cfg = pkg.default_config("heading")
        cell = U.draw_cell(np.random.default_rng([U.SEED, loc, 1]))
        cfg.center_lon, cfg.center_lat, cfg.altitude_limit = lon, lat, U.ALTITUDE_LIMIT
        cfg.init[0].lon_deg, cfg.init[0].lat_geod_deg = lon, lat
        for key in ("v_fps", "w_fps", "p_rad_sec", "q_rad_sec", "r_rad_sec"):
            setattr(cfg.init[0], key, cell[key])
        env = pkg.HipVecEnv(cfg, E, seed=seed)
        ocfg = oracle.config_from_ac(cfg)
        refs = [oracle.OracleEnv(ocfg, pcg64_state=np.random.PCG64(seed + 1000 * i).state) for i in range(E)]
        obs = env.reset()
        robs = np.stack([r.reset() for r in refs])
        assert obs_close(obs, robs, HEADING_OBS_X).all(), (name, "reset", np.abs(obs - robs).max())
        names = env.lib.state_field_names()
        fdm = U.fdm_fields({nm: k for k, nm in enumerate(names) if nm})
        rng = np.random.default_rng([U.SEED, loc, 2])
        u_obs = u_rew = 0.0
        for step in range(steps):
            for e in range(E):
                v = env.get_state(e, 0)
                v[fdm] = refs[e].export_state(0)[fdm]
                env.set_state(e, 0, v)
            if step % U.HOLD == 0:
                act = np.stack([rng.integers(0, n, size=(E, 1)) for n in (41, 41, 41, 30)], axis=-1).astype(np.float32)
            obs, rew, done, info = env.step(act)
            for e in range(E):
                o, r, d, i = refs[e].step(act[e])
                if i[3]:
                    o = refs[e].reset()
                assert bool(done[e, 0, 0]) == bool(d[0]), (name, step, e)
                u_obs = max(u_obs, float((np.abs(obs[e] - o) / (2e-4 + 2e-4 * np.abs(o))).max()))
                u_rew = max(u_rew, abs(rew[e, 0, 0] - r[0]) / (5e-3 + 1e-3 * abs(r[0])))
                assert obs_close(obs[e], o, HEADING_OBS_X).all(), (name, step, e, obs[e], o)
                assert abs(rew[e, 0, 0] - r[0]) <= HEADING_REW_X * (5e-3 + 1e-3 * abs(r[0])), (name, step, e, rew[e, 0, 0], r[0])
        env.close()
        used[name] = (round(u_obs, 3), round(u_rew, 3))
    print("heading: worst multiple of the one-step bounds used (observation: 2x allowed, reward: 1x), per location:", used)
