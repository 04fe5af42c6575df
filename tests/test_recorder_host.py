"""The flight recorder's host side (include/aircombat_record.h, recorder.py, acmi.FrameWriter), no GPU: the column table for the task
shapes, the ACMI state machine that render() and write_acmi share against text assembled by hand from acmi's record functions, and the
episode spans and ring arithmetic."""
import importlib
import os
import re
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def R(pkg):
    return importlib.import_module("aircombat-selfplay_amd.recorder")


@pytest.fixture(scope="module")
def acmi(pkg):
    return importlib.import_module("aircombat-selfplay_amd.acmi")


# (task, A, munition slots, extension) -> what the field list of the header gives
SHAPES = {"heading": (0, 1, 0, False), "singlecombat": (1, 2, 0, False), "singlecombat_shoot": (3, 2, 4, False),
          "scenario1": (5, 2, 2, True), "scenario_nvn_4v4": (6, 8, 2, True)}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_layout_follows_the_field_list(pkg, R, shape):
    task, A, K, ext = SHAPES[shape]
    cols, bytes_af = R.layout(pkg.load_library(), task, A, K, ext)
    want = [("cur_step", "<i4", 1), ("flags", "<i4", 1), ("status", "<i4", 1), ("entity", "<f8", 12)]
    if K:
        want += [("msl_status", "<i4", K), ("msl_model", "<i4", K), ("msl_pose", "<f8", 5 * K)]
    if ext:
        want += [("ext", "<i4", 2)]
    assert cols == want
    # three int32, twelve float64; per slot two int32 and five float64; two int32 extension words
    assert bytes_af == 3 * 4 + 12 * 8 + K * (2 * 4 + 5 * 8) + (2 * 4 if ext else 0)
    assert bytes_af == {"heading": 108, "singlecombat": 108, "singlecombat_shoot": 300, "scenario1": 212, "scenario_nvn_4v4": 212}[shape]
    dt = R.frame_dtype(cols)
    assert dt.itemsize == bytes_af and dt["entity"].shape == (12,)
    if K:
        assert dt["msl_pose"].shape == (K, 5) and dt["msl_status"].shape == (K,)


def test_layout_refuses_shapes_no_handle_has(pkg, R):
    lib = pkg.load_library()
    for bad in ((1, 0, 0, False), (1, 9, 0, False), (1, 2, 5, False), (1, 2, -1, False), (99, 2, 0, False)):
        with pytest.raises(ValueError, match="ac_recorder_layout"):
            R.layout(lib, *bad)


def test_symbols_are_in_the_library_and_the_header(pkg):
    hdr = open(os.path.join(ROOT, "include", "aircombat_record.h")).read()
    declared = set(re.findall(r"\b(ac_recorder_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"ac_recorder_layout", "ac_recorder_create", "ac_recorder_destroy", "ac_recorder_bytes", "ac_recorder_attach",
                        "ac_recorder_detach", "ac_recorder_capture", "ac_recorder_count", "ac_recorder_info", "ac_recorder_read",
                        "ac_recorder_device_ptr"}
    lib = pkg.load_library()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib.path], text=True)
    for sym in declared:
        assert sym in pkg.capi.SIGNATURES and hasattr(lib, sym) and re.search(rf"\bT {sym}\b", exported), sym
    assert pkg.FlightRecorder is importlib.import_module("aircombat-selfplay_amd.recorder").FlightRecorder


def test_layout_struct_matches_the_header(pkg, tmp_path):
    import ctypes as C
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "aircombat_record.h"\n'
                   'int main(){printf("%zu %zu %zu", sizeof(ac_recorder_column_t), sizeof(ac_recorder_layout_t), sizeof(ac_recorder_info_t));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a, b, c = map(int, subprocess.check_output([str(exe)], text=True).split())
    assert (a, b, c) == (C.sizeof(pkg.capi.AcRecorderColumn), C.sizeof(pkg.capi.AcRecorderLayout), C.sizeof(pkg.capi.AcRecorderInfo))


# ---- the shared writer ---------------------------------------------------------------------------------------------------------------

def cfg_of(task, n_agents, n_ego, missiles):
    return types.SimpleNamespace(task=task, n_agents=n_agents, n_ego=n_ego, num_missiles=list(missiles) + [0] * (8 - len(missiles)),
                                 center_lon=120.0, center_lat=60.0, center_alt=0.0, agent_interaction_steps=12, sim_freq=60)


CENTER = (120.0, 60.0, 0.0)


def entity(a, step):
    """distinct, step-dependent values: lon, lat, alt, roll, pitch, yaw (+ six that the records do not use)"""
    return np.array([120.0 + 0.01 * a + 1e-4 * step, 60.0 + 0.02 * a, 6000.0 + 10.0 * a + step, 0.1 * a, 0.05 + 0.001 * step, 1.0 + a] + [0.0] * 6)


NONE = (-1, 0, 0.0, 0.0, 0.0, 0.0, 0.0)    # an empty slot


def msl(status, model, step, a=0):
    return (status, model, 100.0 * step + a, -50.0 * step, 6000.0 + step, 0.01 * step, 0.5 + 0.1 * a)


def frame_text(step, lines, cfg):
    return f"#{step * cfg.agent_interaction_steps / cfg.sim_freq:.2f}\n" + "".join(l + "\n" for l in lines)


def aircraft_lines(acmi, step, A=2):
    return [acmi.aircraft_record(f"{'A' if a < A // 2 else 'B'}0100", "Blue" if a < A // 2 else "Red", entity(a, step)) for a in range(A)]


def test_missile_flies_then_ends(acmi):
    """shoot task, 2 missiles per aircraft: agent 0's first launch is slot 0 = uid A01002; it flies two frames, hits (removal and explosion
    record once, 300 m), and is a bare removal afterwards"""
    cfg = cfg_of(3, 2, 1, [2, 2])
    w = acmi.FrameWriter(cfg, 2)
    assert w.n_slots == [2, 2] and w.radius == 300 and not w.has_chaff
    status = [-1, 0, 0, 1, 1, 1]
    got, want = "", ""
    exploded = False
    for step, st in enumerate(status, start=1):
        m = NONE if st < 0 else msl(st, 0, step)
        got += w.frame(step, [entity(0, step), entity(1, step)], [[m, NONE, NONE, NONE], [NONE] * 4])
        lines = aircraft_lines(acmi, step)
        if st >= 0:
            rec, exploded = acmi.missile_records("A01002", "Blue", st, m[2:5], m[5], m[6], CENTER, exploded, 300, "AIM-9L")
            lines.append(rec)
        want += frame_text(step, lines, cfg)
    assert got == want
    assert got.count("Type=Misc+Explosion") == 1 and got.count("-A01002\n") == 3 and "Radius=300" in got and "Name=AIM-9L" in got
    assert got.count("-A01002\n\n") == 2            # the bare removal carries its own newline


def test_two_launches_in_one_frame_are_ordered_by_step_then_agent(acmi):
    """scenario1: the Red aircraft launched at step 2, both launch a second munition at step 4. env._tempsims keeps first-launch
    order: B01002 (step 2), then A01002 and B01001 (step 4, agent order); slot k of two is uid count 2 - k"""
    cfg = cfg_of(5, 2, 1, [2, 2])
    w = acmi.FrameWriter(cfg, 2)
    assert w.n_slots == [2, 2] and w.radius == 5 and w.has_chaff
    nochaff = [(0, ((0, 0), (0, 0)))] * 2
    got, want = "", ""
    for step in range(1, 6):
        a0 = [msl(0, 1, step, 0) if step >= 4 else NONE, NONE]
        b0 = [msl(0, 2, step, 1) if step >= 2 else NONE, msl(0, 1, step, 1) if step >= 4 else NONE]
        got += w.frame(step, [entity(0, step), entity(1, step)], [a0, b0], nochaff)
        lines = aircraft_lines(acmi, step)
        order = []
        if step >= 2:
            order.append(("B01002", "Red", b0[0], "AIM-9M"))
        if step >= 4:
            order += [("A01002", "Blue", a0[0], "AIM-120B"), ("B01001", "Red", b0[1], "AIM-120B")]
        for uid, color, m, model in order:
            lines.append(acmi.missile_records(uid, color, 0, m[2:5], m[5], m[6], CENTER, False, 5, model)[0])
        want += frame_text(step, lines, cfg)
    assert got == want
    last = got.split("#1.00\n")[1].splitlines()
    assert [l.split(",")[0] for l in last] == ["A0100", "B0100", "B01002", "A01002", "B01001"]


def test_chaff_cloud_keeps_the_release_pose_and_turns_into_its_removal(acmi):
    """scenario1, 2 munitions: agent 0 releases one event against two incoming missiles at step 3 (uids A010012, A010011); the clouds
    keep the pose of step 3, dissolve at step 6 and are removal lines from then on. The words are packed as the kernels pack them."""
    cfg = cfg_of(5, 2, 1, [2, 2])
    w = acmi.FrameWriter(cfg, 2)
    word1 = lambda n_ch, s0, m0: (n_ch << 2) | (s0 << 4) | (m0 << 6)
    assert acmi.chaff_from_words(0, word1(1, 1, 2) | (1 << 5) | (7 << 11)) == (1, ((1, 2), (1, 7)))
    got, want = "", ""
    for step in range(1, 8):
        n_ch, dissolved = (1 if step >= 3 else 0), (1 if step >= 6 else 0)
        chaff = [acmi.chaff_from_words(0x0fffffff, word1(n_ch, dissolved, 2 if n_ch else 0) | (200 << 16)), acmi.chaff_from_words(0, 0)]
        got += w.frame(step, [entity(0, step), entity(1, step)], [[NONE, NONE], [NONE, NONE]], chaff)
        lines = aircraft_lines(acmi, step)
        if step >= 3:
            for uid in ("A010012", "A010011"):
                lines.append(acmi.chaff_record(uid, "Blue", step < 6, tuple(entity(0, 3)[:6])))
        want += frame_text(step, lines, cfg)
    assert got == want
    assert got.count("Name=CHF") == 2 * 3 and got.count("-A010012\n") == 2


def test_a_dropping_cur_step_clears_the_bookkeeping(acmi):
    """an exploded missile and a chaff cloud, then cur_step falls to 0: the next episode starts clean, and a new launch into the same
    slot shows its explosion again"""
    cfg = cfg_of(5, 2, 1, [2, 2])
    w = acmi.FrameWriter(cfg, 2)
    ents = lambda s: [entity(0, s), entity(1, s)]
    chaff1 = [(1, ((0, 1), (0, 0))), (0, ((0, 0), (0, 0)))]
    none = [(0, ((0, 0), (0, 0)))] * 2
    w.frame(5, ents(5), [[msl(0, 1, 5), NONE], [NONE, NONE]], chaff1)
    t6 = w.frame(6, ents(6), [[msl(1, 1, 6), NONE], [NONE, NONE]], chaff1)
    assert "Type=Misc+Explosion" in t6 and "Name=CHF" in t6 and w.exploded == {(0, 0)} and list(w.chaff) == ["A010012"]
    t0 = w.frame(0, ents(0), [[msl(1, 1, 6), NONE], [NONE, NONE]], none)     # the reset frame: stale slot, nothing remembered
    assert w.chaff == {} and "CHF" not in t0
    m = msl(1, 1, 6)
    rec, _ = acmi.missile_records("A01002", "Blue", 1, m[2:5], m[5], m[6], CENTER, False, 5, "AIM-120B")
    assert t0 == frame_text(0, aircraft_lines(acmi, 0) + [rec], cfg)
    # an equal cur_step (two reset frames in a row) clears as well
    w.frame(0, ents(0), [[NONE, NONE], [NONE, NONE]], none)
    assert w.exploded == set() and w.first == {}


def test_acmi_text_feeds_the_writer_from_structured_frames(pkg, R, acmi):
    """write_acmi's path from a frames array: the same text as the writer fed by hand"""
    cfg = cfg_of(5, 2, 1, [2, 2])
    cols, _ = R.layout(pkg.load_library(), 5, 2, 2, True)
    fr = np.zeros((3, 2), dtype=R.frame_dtype(cols))
    w = acmi.FrameWriter(cfg, 2)
    want = acmi.HEADER
    for i, step in enumerate((4, 5, 6)):
        fr["cur_step"][i] = step
        fr["msl_status"][i] = -1
        for a in range(2):
            fr["entity"][i, a] = entity(a, step)
        m = msl(0 if step < 6 else 2, 2, step)
        fr["msl_status"][i, 0, 1], fr["msl_model"][i, 0, 1], fr["msl_pose"][i, 0, 1] = m[0], m[1], m[2:]
        fr["ext"][i, 1] = (0, (1 << 2) | (1 << 6))
        want += w.frame(step, [entity(0, step), entity(1, step)], [[NONE, m], [NONE, NONE]], [(0, ((0, 0), (0, 0))), (1, ((0, 1), (0, 0)))])
    got = R.acmi_text(cfg, fr)
    assert got == want and "Name=AIM-9M" in got and "B010012,T=" in got and "Radius=5" in got


# ---- spans and ring arithmetic -------------------------------------------------------------------------------------------------------

def test_episode_spans(R):
    assert R.episode_spans([]) == []
    assert R.episode_spans([0, 1, 2, 3]) == [(0, 3)]
    assert R.episode_spans([0, 1, 2, 0, 1, 0, 0, 1]) == [(0, 2), (3, 4), (5, 5), (6, 7)]
    # a ring whose oldest frame is frame 40, in the middle of an episode: the first span is that episode's tail
    assert R.episode_spans([7, 8, 9, 0, 1, 2, 3, 0], first_frame=40) == [(40, 42), (43, 46), (47, 47)]
    # the frame of the step that ended an episode already shows cur_step 0 (auto-reset); a reset() right after it gives 0 again
    assert R.episode_spans([3, 4, 0, 0, 1], first_frame=10) == [(10, 11), (12, 12), (13, 14)]


@pytest.mark.parametrize("count", [0, 5, 8, 11])
def test_ring_arithmetic(R, count):
    F = 8
    lo, hi = R.readable_range(count, F)
    assert (lo, hi) == {0: (0, 0), 5: (0, 5), 8: (0, 8), 11: (3, 11)}[count]
    assert hi - lo <= F
    # every readable frame has a slot of its own, and frame f sits in slot f % F
    slots = [R.ring_slot(f, F) for f in range(lo, hi)]
    assert len(set(slots)) == len(slots) and all(s == f % 8 for s, f in zip(slots, range(lo, hi)))
    if count:
        assert R.check_span(count, F, lo, hi - 1) == (lo, hi - lo)
        assert R.check_span(count, F, hi - 1, hi - 1) == (hi - 1, 1)
        with pytest.raises(ValueError, match="not been captured"):
            R.check_span(count, F, lo, hi)
        with pytest.raises(ValueError, match="empty span"):
            R.check_span(count, F, hi - 1, hi - 2)
    else:
        with pytest.raises(ValueError, match="not been captured"):
            R.check_span(count, F, 0, 0)
    if lo > 0:
        with pytest.raises(ValueError, match="overwritten"):
            R.check_span(count, F, lo - 1, hi - 1)
    with pytest.raises(ValueError):
        R.check_span(count, F, -1, 0)
