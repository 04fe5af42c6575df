"""CPU-side checks of the product: the C-ABI library loads and exports every symbol include/aircombat.h declares, the
ctypes structs match the header, the YAML -> ac_config mapping follows the reference's conventions, and the product
never touches the oracle. No compute calls (no GPU here)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(pkg):
    hdr = "".join(open(os.path.join(ROOT, "include", f)).read() for f in sorted(os.listdir(os.path.join(ROOT, "include"))) if f.endswith(".h"))
    declared = set(re.findall(r"\b(ac_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(pkg.capi.SIGNATURES), declared ^ set(pkg.capi.SIGNATURES)
    lib = pkg.load_library()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib.path], text=True)
    for sym in declared:
        assert re.search(rf"\bT {sym}\b", exported), sym
    assert lib.ac_version().startswith(b"aircombat-hip")
    names = lib.state_field_names()
    assert names[:3] == ["rx", "ry", "rz"] and "status" in names and "cur_step" in names
    assert len([n for n in names if n]) <= pkg.capi.AC_STATE_LEN


def test_config_struct_layout_matches_header(pkg, tmp_path):
    """sizeof(ac_config_t) as the C compiler sees it == ctypes.sizeof(AcConfig)."""
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "aircombat.h"\n#include "aircombat_buffer.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu", sizeof(ac_config_t), sizeof(ac_init_state_t), sizeof(ac_buffer_config_t), '
                   'sizeof(ac_buffer_step_t), sizeof(ac_buffer_batch_t));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a, b, c, d, e = map(int, subprocess.check_output([str(exe)], text=True).split())
    assert a == C.sizeof(pkg.AcConfig) and b == C.sizeof(pkg.AcInitState)
    assert (c, d, e) == (C.sizeof(pkg.capi.AcBufferConfig), C.sizeof(pkg.capi.AcBufferStep), C.sizeof(pkg.capi.AcBufferBatch))


def test_missing_library_fails_loudly(pkg, tmp_path):
    with pytest.raises(pkg.HipExtensionMissing):
        pkg.capi.Lib(str(tmp_path / "nope.so"))


def test_create_without_gpu_reports_error_not_fallback(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="ac_create failed"):
        pkg.HipVecEnv(pkg.default_config("singlecombat"), 2)


def test_yaml_mapping_follows_reference_conventions(pkg, tmp_path):
    y = tmp_path / "s.yaml"
    y.write_text("""
task: singlecombat
sim_freq: 60
agent_interaction_steps: 6
max_steps: 9000
altitude_limit: 2400
acceleration_limit_z: 8.5
aircraft_configs: {
  A0100: {color: Blue, model: f16, init_state: {ic_long_gc_deg: 120.0, ic_lat_geod_deg: 60.0, ic_h_sl_ft: 20000, ic_psi_true_deg: 0, ic_u_fps: 800.0}, missile: 2},
  B0100: {color: Red, model: f16, init_state: {ic_h_sl_ft: 99999, ic_lat_geod_deg: 60.1, ic_long_gc_deg: 120.5, ic_psi_true_deg: 180.0, ic_u_fps: 800.0}, missile: 1}
}
battle_field_center: [120.0, 60.0, 0.0]
PostureReward_scale: 15.0
PostureReward_potential: true
EventDrivenReward_potential: true
""")
    cfg = pkg.config_from_yaml(str(y))
    assert cfg.task == 1 and cfg.n_agents == 2 and cfg.n_ego == 1
    assert cfg.altitude_limit == 2400 and cfg.acc_limit_z == 8.5 and cfg.acc_limit_x == 10.0
    assert cfg.init[1].psi_deg == 180.0 and cfg.init[1].h_sl_ft == 85000           # catalogue clip of ic_h_sl_ft
    assert cfg.init[0].v_fps == 0.0 and cfg.init[0].u_fps == 800.0                   # simulatior.py:192-208 defaults
    assert cfg.num_missiles[0] == 2 and cfg.num_missiles[1] == 1
    assert cfg.posture_scale == 15.0 and cfg.posture_potential == 1 and cfg.altitude_potential == 0
    assert cfg.alt_safe == 4.0 and cfg.alt_kv == 0.2 and cfg.min_attack_interval == 125  # class defaults
    with pytest.raises(NotImplementedError):
        pkg.config_from_yaml(str(y), task="scenario9")


def test_product_never_imports_the_oracle():
    pkgdir = os.path.join(ROOT, "aircombat-selfplay_amd")
    for dirpath, _, files in os.walk(pkgdir):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle" not in text.lower() or f == "f16_tables.h", (f, "mentions the oracle")
    lib = os.path.join(pkgdir, "libaircombat_hip.so")
    if os.path.exists(lib):
        needed = subprocess.check_output(["readelf", "-d", lib], text=True)
        assert "liboracle" not in needed


def test_generated_table_copies_are_in_sync():
    a = open(os.path.join(ROOT, "oracle", "f16_tables.h")).read()
    b = open(os.path.join(ROOT, "aircombat-selfplay_amd", "csrc", "f16_tables.h")).read()
    assert a == b


def test_two_wave_tick_pieces_are_generated_from_the_current_tick():
    """csrc/f16_split.hpp holds the statements of tick() cut into the pieces of the three-wave kernels; it must be what
    tools/gen_split_tick.py makes of the current f16_device.hpp, so that the two kernel forms compute the same arithmetic."""
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_split_tick.py"), "--check"]).returncode == 0


def test_curriculum_spawn_matches_reference_table():
    """Host-side restatement of calculate_coordinates_heading_by_curriculum against the fixture generated from the reference,
    and the *_curriculum task names resolving to their base task with the angle-0 spawn."""
    import numpy as np
    import aircombat_selfplay_amd as pkg
    from aircombat_selfplay_amd.config import curriculum_spawn, config_from_dict
    t = np.load(os.path.join(os.path.dirname(__file__), "golden", "curriculum_spawn.npz"))["table"]
    for a in range(181):
        assert np.allclose(curriculum_spawn(60.1, 120.0, 11.119, a), t[a], rtol=0, atol=1e-12), a
    base = pkg.default_config("scenario1")
    data = {"task": "scenario1_curriculum", "sim_freq": 60, "agent_interaction_steps": 6,
            "aircraft_configs": {"A0100": {"color": "Blue", "missile": 2, "init_state": {}}, "B0100": {"color": "Red", "missile": 2, "init_state": {}}}}
    cfg = config_from_dict(data, hierarchical=True)
    assert cfg.task == base.task and cfg.hierarchical == 1
    assert abs(cfg.init[0].lat_geod_deg - t[0][0]) < 1e-12 and cfg.init[0].psi_deg == 0 and cfg.init[1].lat_geod_deg == 60.1
    data["curriculum_angle"] = 45
    cfg = config_from_dict(data)
    assert abs(cfg.init[0].lon_deg - t[45][1]) < 1e-12 and cfg.init[0].psi_deg == 90


def test_acmi_records_and_neu_inverse():
    """Host-side ACMI formatting (BaseSimulator.log / MissileSimulator.log) and the NEU -> geodetic inverse used for missile
    records, against the CPU checker's restatement of pymap3d (round trip < 1 mm, 1e-9 deg)."""
    import importlib
    import numpy as np
    import aircombat_selfplay_amd as pkg
    acmi = importlib.import_module(pkg.__name__ + ".acmi")
    from oracle import oracle as O
    L = O.lib()
    dp = C.POINTER(C.c_double)
    L.or_neu2lla.argtypes = [C.c_double] * 6 + [dp]
    rng = np.random.default_rng(3)
    for _ in range(200):
        n, e, u = rng.uniform(-60000, 60000), rng.uniform(-60000, 60000), rng.uniform(0, 15000)
        out = np.zeros(3)
        L.or_neu2lla(n, e, u, 120.0, 60.0, 0.0, out.ctypes.data_as(dp))
        got = acmi.neu_to_lla(n, e, u, 120.0, 60.0, 0.0)
        assert abs(got[0] - out[0]) < 1e-9 and abs(got[1] - out[1]) < 1e-9 and abs(got[2] - out[2]) < 1e-3, (got, out)
    rec = acmi.aircraft_record("A0100", "Blue", [120.0, 60.0, 6096.0, 0.0, 0.1, 1.0])
    assert rec.startswith("A0100,T=120.0|60.0|6096.0|0.0|") and rec.endswith("Name=F16,Color=Blue")
    r, boom = acmi.missile_records("A01001", "Blue", 1, (100.0, 50.0, 6000.0), 0.0, 0.5, (120.0, 60.0, 0.0), False, 300)
    assert boom and r.startswith("-A01001\nA01001F,T=") and "Type=Misc+Explosion" in r
    r2, boom2 = acmi.missile_records("A01001", "Blue", 1, (100.0, 50.0, 6000.0), 0.0, 0.5, (120.0, 60.0, 0.0), True, 300)
    assert r2 == "-A01001\n" and boom2          # the reference's removal message carries its own newline (simulatior.py:547-548)


def test_lazy_infos_equal_the_reference_info_dicts(pkg):
    """`infos` of VecEnv.step builds its dicts on access: element by element it must equal what the workers' dicts hold
    (env_wrappers.py:276-282): current_step always, done_condition on an episode end, heading_turn_counts with UnreachHeading."""
    import importlib
    import numpy as np
    ve = importlib.import_module("aircombat-selfplay_amd.vec_env")
    codes = np.array([[3, 0, 0, 0], [7, 8, 2, 1], [9, 1, 0, 1], [12, 7, 0, 1]], dtype=np.int32)
    infos = ve.LazyInfos(codes)
    assert len(infos) == 4 and infos.shape == (4,)
    assert infos[0] == {"current_step": 3}
    assert infos[1] == {"current_step": 7, "done_condition": ve.DONE_MESSAGES[8], "heading_turn_counts": 2}
    assert infos[-1]["done_condition"] == ve.DONE_MESSAGES[7] and "heading_turn_counts" not in infos[-1]
    assert [i for i in infos if "heading_turn_counts" in i] == [infos[1]]          # runner/jsbsim_runner.py:55-57
    arr = np.asarray(infos)
    assert arr.dtype == object and arr.shape == (4,) and arr[2] == infos[2]
    assert infos[1:3] == [infos[1], infos[2]]
    with pytest.raises(IndexError):
        infos[4]


def test_acmi_records_match_the_reference_log_text(pkg):
    """the Tacview records against the text the reference's own log() methods produced for a scripted sequence
    (tests/golden/acmi_records.npz, written by make_golden.py from BaseSimulator / MissileSimulator / ChaffSimulator.log): aircraft and
    chaff records must be the same strings (same float64 inputs, same formatting); a missile record is rebuilt from its NEU position
    through NEU2LLA, so its numbers are compared to 1e-9 deg / 1e-6 m and everything else as text. Frame layout of BaseEnv.render."""
    import importlib
    import numpy as np
    acmi = importlib.import_module(pkg.__name__ + ".acmi")
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acmi_records.npz"))
    center = tuple(z["center"])
    radius = int(z["missile_radius"][0])
    exploded = False
    chaff_pose = None
    seen_explosion = seen_removed_chaff = False
    for f, (text, row) in enumerate(zip(z["frames"], z["inputs"])):
        want = str(text).split("\n")
        assert want[0] == f"#{(f + 1) * 0.1:.2f}"
        got = [want[0]]
        a_pose, b_pose = row[0:6], row[6:12]
        got.append(acmi.aircraft_record("A0100", "Blue", a_pose))
        got.append(acmi.aircraft_record("B0100", "Red", b_pose))
        status, neu, rpy, chaff_state = int(row[12]), row[13:16], row[16:19], int(row[19])
        rec, exploded = acmi.missile_records("A01002", "Blue", status, neu, rpy[1], rpy[2], center, exploded, radius, "AIM-120B")
        got.append(rec)
        if chaff_state:
            if chaff_pose is None:
                chaff_pose = tuple(b_pose)          # the release happened at the end of this frame's env step
            got.append(acmi.chaff_record("B010012", "Red", chaff_state == 1, chaff_pose))
        got_text = "\n".join(got) + "\n"
        glines, wlines = got_text.split("\n"), str(text).split("\n")
        assert len(glines) == len(wlines), (f, got_text, str(text))
        for g, w in zip(glines, wlines):
            if g == w:
                continue
            # a missile record: same fields, position rebuilt from NEU
            gp, wp = g.split(","), w.split(",")
            assert gp[0] == wp[0] and gp[2:] == wp[2:], (f, g, w)
            gv, wv = [float(v) for v in gp[1][2:].split("|")], [float(v) for v in wp[1][2:].split("|")]
            assert abs(gv[0] - wv[0]) < 1e-9 and abs(gv[1] - wv[1]) < 1e-9 and abs(gv[2] - wv[2]) < 1e-6 and gv[3:] == wv[3:], (f, g, w)
        seen_explosion |= "Type=Misc+Explosion" in got_text
        seen_removed_chaff |= "-B010012" in got_text
    assert seen_explosion and seen_removed_chaff and exploded


def test_controller_products_split_into_two_fp16_pieces(pkg):
    """The arithmetic claim behind controller8_kernel (host side of it, no GPU): x ~ hi + lo with two fp16 pieces (round-to-nearest
    each, 11 significant bits), |x - hi - lo| <= 2^-22 |x| for the magnitudes the network sees (2^-25 absolute once lo is an fp16
    subnormal); and the three kept product terms reproduce the exact product to 2^-21 of it (worst case)."""
    import ctypes as C
    import numpy as np
    lib = pkg.load_library()
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal(20000) * 10.0 ** rng.integers(-3, 3, 20000), [0.0, -0.0, 1.0, -1.0, 60000.0, -60000.0, 0.1, 1.0 / 3.0]]).astype(np.float32)
    x = x[np.abs(x) < 65000.0]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    hi, lo = np.empty_like(x), np.empty_like(x)
    assert lib.dll.ac_split_f16x2(p(x), x.size, p(hi), p(lo)) == 0
    for piece in (hi, lo):
        assert (piece.astype(np.float16).astype(np.float32) == piece).all()     # an fp16 value each
    assert (hi == x.astype(np.float16).astype(np.float32)).all()                  # round to nearest even, like numpy's
    f = lambda a: a.astype(np.float64)
    left = np.abs(f(x) - f(hi) - f(lo))
    assert (left <= np.maximum(2.0 ** -22 * np.abs(f(x)), 2.0 ** -25)).all()
    y = rng.permutation(x)
    yh, yl = np.empty_like(y), np.empty_like(y)
    lib.dll.ac_split_f16x2(p(y), y.size, p(yh), p(yl))
    kept = f(hi) * f(yh) + f(hi) * f(yl) + f(lo) * f(yh)
    exact = f(x) * f(y)
    ok = (np.abs(f(x)) > 0.125) & (np.abs(f(y)) > 0.125)                          # (both lo pieces normal)
    rel = np.abs(kept - exact)[ok] / np.abs(exact)[ok]
    assert rel.max() <= 2.0 ** -21 * 1.01, rel.max()    # two roundings of 2^-22 each + the dropped lo * lo (<= 2^-22)
    assert np.median(rel) <= 2.0 ** -23
    # a non-finite weight or activation stays non-finite (the step's state probe reports it; nothing is laundered into a number)
    bad = np.array([np.nan, np.inf, -np.inf, 1e9], dtype=np.float32)
    bh, bl = np.empty_like(bad), np.empty_like(bad)
    lib.dll.ac_split_f16x2(p(bad), 4, p(bh), p(bl))
    with np.errstate(invalid="ignore"):
        assert not np.isfinite(bh + bl).any()          # (1e9 is beyond fp16: it saturates to inf rather than wrap to something plausible)


def test_multiplecombat_missile_task_names_resolve(pkg):
    """The three MultipleCombat missile classes no env of the reference constructs (multiplecombat_with_missile_task.py:13-216) have names of
    this package's own: the rule-based one is AC_TASK_DODGE_MISSILE with the NvN aircraft block, the shoot one MULTICOMBAT with the paired-enemy
    observation; `hierarchical_*` sets the controller form."""
    from aircombat_selfplay_amd.capi import AC_TASK_DODGE_MISSILE, AC_TASK_MULTICOMBAT
    d = pkg.default_config("multiplecombat_dodge_missile")
    assert (d.task, d.n_agents, d.n_ego, d.legacy_obs, d.hierarchical) == (AC_TASK_DODGE_MISSILE, 4, 2, 1, 0)
    assert list(d.num_missiles)[:4] == [2, 2, 2, 2] and d.min_attack_interval == 125 and d.max_attack_distance == 14000
    h = pkg.default_config("hierarchical_multiplecombat_dodge_missile")
    assert (h.task, h.n_agents, h.legacy_obs, h.hierarchical) == (AC_TASK_DODGE_MISSILE, 4, 1, 1)
    s8 = pkg.default_nvn_config(4, task="multiplecombat_shoot")
    assert (s8.task, s8.n_agents, s8.n_ego, s8.legacy_obs, s8.hierarchical) == (AC_TASK_MULTICOMBAT, 8, 4, 1, 0)
    with pytest.raises(NotImplementedError):
        pkg.default_nvn_config(2, task="multiplecombat_no_such_task")

