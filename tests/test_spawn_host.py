"""The spawn curriculum without a GPU (include/aircombat_spawn.h, csrc/spawn_bank.hpp, spawn.py): the bank's rows against the
reference's table, the ctypes structs against the header, the per-env rule (the body the spawn kernel runs, compiled for the host)
against a numpy float32 twin bit for bit, the keyed draws, and the refusals that need no device."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import spawn_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_names_are_exported(pkg):
    for name in ("SpawnCurriculum", "curriculum_bank"):
        assert name in pkg.__all__ and getattr(pkg, name).__name__ == name
    assert hasattr(pkg.HipVecEnv, "spawn_curriculum") and hasattr(pkg.HipShareVecEnv, "stop_curriculum")


def test_bank_rows_match_the_reference_table(pkg):
    t = np.load(os.path.join(os.path.dirname(__file__), "golden", "curriculum_spawn.npz"))["table"]
    cfg2, cfg4 = pkg.default_config("scenario1"), pkg.default_config("scenario_nvn")
    before = bytes(cfg2), bytes(cfg4)
    b2, b4 = pkg.curriculum_bank(cfg2, range(181)), pkg.curriculum_bank(cfg4)
    assert (bytes(cfg2), bytes(cfg4)) == before                      # the config is left alone
    assert len(b2) == len(b4) == 181 and all(len(r) == 2 for r in b2) and all(len(r) == 4 for r in b4)
    close = lambda x, y: abs(x - y) <= 1e-12
    for a in range(181):
        blue, red = b2[a]
        assert close(blue.lat_geod_deg, t[a][0]) and close(blue.lon_deg, t[a][1]) and blue.psi_deg == t[a][2], a
        assert (red.lat_geod_deg, red.lon_deg, red.psi_deg) == (60.1, 120.0, 0.0)
        r = b4[a]
        assert close(r[0].lat_geod_deg, t[a][0]) and close(r[0].lon_deg, t[a][1]) and r[0].psi_deg == t[a][2], a
        # the wingman's circle is centred 0.01 deg of longitude further east: the same latitude and heading, the longitude shifted
        assert close(r[1].lat_geod_deg, t[a][0]) and close(r[1].lon_deg, t[a][1] + 0.01) and r[1].psi_deg == t[a][2], a
        assert [(x.lat_geod_deg, x.lon_deg, x.psi_deg) for x in r[2:]] == [(60.1, 120.0, 0.0), (60.1, 120.01, 0.0)]
        for ic in list(b2[a]) + list(r):
            assert (ic.h_sl_ft, ic.u_fps, ic.v_fps, ic.w_fps) == (20000.0, 800.0, 0.0, 0.0)
    # dict rows with the YAML's keys pack like AcInitState rows
    S = importlib.import_module("aircombat-selfplay_amd.spawn")
    flat, K = S.pack_rows([[{"ic_long_gc_deg": 120.25, "ic_h_sl_ft": 99999}, b2[7][1]]], 2)
    assert K == 1 and flat[0].lon_deg == 120.25 and flat[0].h_sl_ft == 85000 and flat[0].u_fps == 800.0 and bytes(flat[1]) == bytes(b2[7][1])
    with pytest.raises(ValueError, match="has 1 aircraft"):
        S.pack_rows([[b2[0][0]]], 2)


def test_struct_layout_matches_header(pkg, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "aircombat_spawn.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu %d %d", sizeof(ac_spawn_config_t), sizeof(ac_spawn_state_t), sizeof(ac_spawn_post_step_t), '
                   'offsetof(ac_spawn_config_t, seed), offsetof(ac_spawn_post_step_t, cfg), offsetof(ac_spawn_post_step_t, index), '
                   '(int)AC_SPAWN_MAX_BANK, (int)AC_SPAWN_MAX_WINDOW);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a, b, c, d, e, f, g, h = map(int, subprocess.check_output([str(exe)], text=True).split())
    K = pkg.capi
    assert (a, b, c) == (C.sizeof(K.AcSpawnConfig), C.sizeof(K.AcSpawnState), C.sizeof(K.AcSpawnPostStep))
    assert (d, e, f) == (K.AcSpawnConfig.seed.offset, K.AcSpawnPostStep.cfg.offset, K.AcSpawnPostStep.index.offset)
    assert (g, h) == (K.AC_SPAWN_MAX_BANK, K.AC_SPAWN_MAX_WINDOW) == (1024, 32)
    assert (K.AC_SPAWN_FIXED, K.AC_SPAWN_AUTO, K.AC_SPAWN_AT, K.AC_SPAWN_UPTO) == (0, 1, 0, 1)


def _streams(rng, E, A, steps):
    """rewards on a coarse and a fine grid (sums that round and sums that do not), reset flags about every third step"""
    rew = (rng.integers(-40, 41, size=(steps, E, A)) * 0.37).astype(np.float32) + rng.standard_normal((steps, E, A)).astype(np.float32) * np.float32(1e-3)
    info = np.zeros((steps, E, 4), dtype=np.int32)
    info[..., 0] = rng.integers(0, 100, size=(steps, E))
    info[..., 3] = rng.random((steps, E)) < 0.35
    return rew, info


@pytest.mark.parametrize("window", [1, 2, 20, 32])
@pytest.mark.parametrize("n_ego", [1, 2, 4])
@pytest.mark.parametrize("E", [1, 5, 33])
def test_rule_equals_the_numpy_twin(pkg, E, n_ego, window):
    A, K, steps = 2 * n_ego, 4, 160
    rng = np.random.default_rng(1000 * E + 10 * n_ego + window)
    for mode, sample in (("auto", "at"), ("auto", "upto"), ("fixed", "upto")):
        min_wins = max(1, (3 * window + 3) // 4)
        cfg = SU.spawn_cfg(pkg, mode, sample, window, min_wins, win_return=0.5, seed=77 + E)
        twin = SU.Twin(E, K, n_ego, mode, sample, window, min_wins, 0.5, 77 + E)
        arrays = {k: v.copy() for k, v in twin.arrays().items()}
        rew, info = _streams(rng, E, A, steps)
        advanced = False
        for t in range(steps):
            stage_was = arrays["stage"].copy()
            if t == 50:                  # out-of-range stages, as a caller's scribble leaves them: clamped where they are used
                for a in (twin.stage, arrays["stage"]):
                    a[::2] = 1000
                    a[1::3] = -5
            if t == 90:                  # the form queued behind a reset: every env ends its episode unscored
                want = twin.step(None, None, all_envs=True)
                got = SU.host_step(pkg, cfg, K, n_ego, rew[t], info[t], arrays, all_envs=True)
                assert (want >= 0).all()
            else:
                want = twin.step(rew[t], info[t])
                got = SU.host_step(pkg, cfg, K, n_ego, rew[t], info[t], arrays)
            assert SU.same(got, want), (mode, sample, t)
            assert ((got >= -1) & (got < K)).all()
            advanced |= bool((arrays["stage"] != stage_was).any())
            for k in SU.FIELDS:
                assert SU.same(arrays[k], twin.arrays()[k]), (mode, sample, t, k)
        assert (arrays["episode"] > 0).all()
        if mode == "auto" and window == 1:
            # the stream's wins carry envs up the bank, the top stage holds, and a scribbled stage comes back into it at its next advance
            assert advanced and set(arrays["stage"].tolist()) <= {K - 1, -5, -4, -3, 1000} | set(range(K))
            assert (arrays["stage"] == K - 1).any()


def test_auto_rule_advances_saturates_and_clears(pkg):
    """a hand-made stream: two wins in a window of two advance, a loss does not, the last stage holds"""
    K, E = 3, 2
    cfg = SU.spawn_cfg(pkg, "auto", "at", window=2, min_wins=2, win_return=1.0)
    twin = SU.Twin(E, K, 1, "auto", "at", 2, 2, 1.0)
    arrays = {k: v.copy() for k, v in twin.arrays().items()}
    end = np.array([[0, 0, 0, 1], [0, 0, 0, 1]], dtype=np.int32)
    run = np.zeros((2, 4), dtype=np.int32)
    stages = []
    for t in range(12):
        rew = np.array([[0.5, 9.0], [0.5 if t % 4 < 3 else -3.0, 9.0]], dtype=np.float32)      # env 0 always wins its two-step episodes, env 1 loses every other
        info = end if t % 2 else run
        assert SU.same(SU.host_step(pkg, cfg, K, 1, rew, info, arrays), twin.step(rew, info))
        stages.append(arrays["stage"].tolist())
    assert stages[3] == [1, 0] and stages[7] == [2, 0] and stages[11] == [2, 0]
    # (env 0's sixth win saturates at the last stage and still clears its record; env 1 never has two wins in a row)
    assert arrays["played"].tolist() == [0, 6] and arrays["wins"].tolist() == [0, 0b101010] and arrays["return_sum"].tolist() == [0.0, -4.5]
    for k in SU.FIELDS:
        assert SU.same(arrays[k], twin.arrays()[k]), k


def test_draws_stay_in_range_and_are_a_function_of_their_key(pkg):
    lib = pkg.load_library()
    S = importlib.import_module("aircombat-selfplay_amd.spawn")
    seed = 12345
    seen = set()
    for env in range(64):
        for ep in range(1, 5):
            k = S.draw(lib, seed, env, ep, 2)
            assert 0 <= k <= 2 and k == S.draw(lib, seed, env, ep, 2) == SU.draw(seed, env, ep, 2)
            seen.add(k)
            assert S.draw(lib, seed, env, ep, 0) == 0
    assert seen == {0, 1, 2}                                             # a condition on the seed the GPU tests use, checked here
    table = lambda s: [S.draw(lib, s, e, p, 1023) for e in range(8) for p in range(8)]
    assert table(seed) != table(seed + 1) and max(table(seed)) <= 1023
    assert [S.draw(lib, seed, e, 1, 1023) for e in range(32)] != [S.draw(lib, seed, e, 2, 1023) for e in range(32)]
    for st in (1, 6, 180, 1023):                                         # roughly uniform: every quarter of [0, stage] is hit
        ks = np.array([S.draw(lib, 9, e, 3, st) for e in range(400)])
        assert ks.min() >= 0 and ks.max() <= st
        assert set(ks.tolist()) == {0, 1} if st == 1 else (np.bincount(ks * 4 // (st + 1), minlength=4) > 50).all()
        assert all(int(k) == SU.draw(9, e, 3, st) for e, k in enumerate(ks))
    with pytest.raises(ValueError, match="stage must be in"):
        S.draw(lib, seed, 0, 0, 1024)


def test_refusals_that_need_no_device(pkg):
    lib, K = pkg.load_library(), pkg.capi
    cfg = pkg.default_config("singlecombat")
    rows = pkg.curriculum_bank(cfg, (0, 45, 90))
    S = importlib.import_module("aircombat-selfplay_amd.spawn")
    flat, n = S.pack_rows(rows, 2)
    good = SU.spawn_cfg(pkg, "auto", "upto", 20, 18, 3.0)
    check = lambda task, A, init, k, c: (lib.ac_spawn_check(task, A, init, k, C.byref(c)), lib.last_error())
    assert check(cfg.task, 2, flat, n, good)[0] == 0
    rc, msg = check(K.AC_TASK_HEADING, 1, flat, 3, good)
    assert rc == -1 and "no reset template" in msg
    for k in (0, -1, 1025):
        rc, msg = check(cfg.task, 2, None, k, good)
        assert rc == -1 and "K must be in 1 .. 1024" in msg
    assert check(cfg.task, 2, None, 1024, good)[0] == 0
    for field, value, what in (("lat_geod_deg", 89.5, "latitude"), ("h_sl_ft", 90000.0, "altitude"), ("u_fps", float("nan"), "non-finite"),
                               ("psi_deg", float("inf"), "non-finite")):
        bad, _ = S.pack_rows(rows, 2)
        setattr(bad[2 * 1 + 1], field, value)                            # entry 1, aircraft 1
        rc, msg = check(cfg.task, 2, bad, n, good)
        assert rc == -1 and "bank entry 1, aircraft 1" in msg and what in msg, msg
    for window, min_wins, what in ((0, 1, "window must be in 1 .. 32"), (33, 1, "window must be in 1 .. 32"), (20, 0, "min_wins must be in 1 .. window"),
                                   (20, 21, "min_wins must be in 1 .. window")):
        rc, msg = check(cfg.task, 2, flat, n, SU.spawn_cfg(pkg, "fixed", "at", window, min_wins))
        assert rc == -1 and what in msg, msg
    for wr in (float("nan"), float("inf")):
        rc, msg = check(cfg.task, 2, flat, n, SU.spawn_cfg(pkg, "auto", "at", 20, 18, wr))
        assert rc == -1 and "finite win_return" in msg
    assert check(cfg.task, 2, flat, n, SU.spawn_cfg(pkg, "fixed", "at", 20, 18, float("nan")))[0] == 0       # fixed mode never looks at it
    c = SU.spawn_cfg(pkg)
    c.mode = 2
    assert check(cfg.task, 2, flat, n, c)[0] == -1 and "unknown mode" in lib.last_error()
    # the Python surface refuses what it can tell by itself, and computes min_wins
    with pytest.raises(ValueError, match="needs win_return"):
        S.spawn_config(mode="auto")
    with pytest.raises(ValueError, match="mode must be"):
        S.spawn_config(mode="sometimes")
    with pytest.raises(ValueError, match="sample must be"):
        S.spawn_config(sample="below")
    assert S.spawn_config(window=20, win_rate=0.9).min_wins == 18 and S.spawn_config(window=32, win_rate=1.0).min_wins == 32
    assert S.spawn_config(window=3, win_rate=0.5).min_wins == 2 and S.spawn_config(window=10, win_rate=0.3).min_wins == 3
    # null arguments and a null bank
    assert lib.ac_spawn_attach(None, flat, n, C.byref(good), C.byref(C.c_void_p())) == -1 and "null argument" in lib.last_error()
    assert lib.ac_spawn_detach(None) == -1 and lib.ac_spawn_set_config(None, C.byref(good)) == -1
    assert lib.ac_spawn_state(None, C.byref(K.AcSpawnState())) == -1
    p = K.AcSpawnPostStep()
    p.E, p.A, p.n_ego, p.K, p.cfg = 1, 2, 1, 1, good
    assert lib.ac_spawn_post_step_host(C.byref(p)) == -1 and "null array" in lib.last_error()
