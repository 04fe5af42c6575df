"""Snapshot header handling on the host (no GPU): encode / decode, the checks EnvSnapshot.from_bytes makes, and the new C-ABI symbols
being exported and declared."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ac_snapshot_bytes", "ac_snapshot_header", "ac_snapshot_save", "ac_snapshot_load", "ac_snapshot_save_host", "ac_snapshot_load_host",
       "ac_clone_envs", "ac_snapshot_load_envs", "ac_get_obs", "ac_snapshot_checksum")


def header(pkg, **kw):
    h = {"version": pkg.load_library().ac_version().decode(), "task": 1, "E": 4096, "A": 2, "msl_slots": 0, "obs_dim": 15, "act_dim": 4,
         "act_low": 4, "ctl_precision": 0, "hierarchical": 0, "n_sections": 3, "config_hash": 0x0123456789ABCDEF,
         "offsets": [1024, 2048, 4096], "bytes": [1000, 2000, 8]}
    h["total_bytes"] = 4352
    h.update(kw)
    return h


def test_snapshot_symbols_exported_and_declared(pkg):
    hdr = open(os.path.join(ROOT, "include", "aircombat.h")).read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.load_library().path], text=True)
    for sym in NEW:
        assert re.search(rf"\b{sym}\s*\(", hdr), sym
        assert sym in pkg.capi.SIGNATURES, sym
        assert re.search(rf"\bT {sym}\b", exported), sym


def test_header_struct_matches_c(pkg, tmp_path):
    """the Python decoder's offsets against the C struct (csrc/snapshot.hpp) as the host compiler lays it out"""
    src = tmp_path / "h.cpp"
    body = open(os.path.join(ROOT, "aircombat-selfplay_amd", "csrc", "snapshot.hpp")).read()
    struct = re.search(r"enum \{ AC_SNAP_MAGIC.*?\n.*?struct AcSnapHeader \{.*?\n\};", body, re.S).group(0)
    src.write_text("#include <stdint.h>\n#include <stddef.h>\n#include <stdio.h>\n" + struct +
                   '\nint main(){printf("%zu %zu %zu %zu %zu", sizeof(AcSnapHeader), offsetof(AcSnapHeader, task), offsetof(AcSnapHeader, config_hash),'
                   ' offsetof(AcSnapHeader, offset), offsetof(AcSnapHeader, bytes));return 0;}\n')
    exe = tmp_path / "h"
    subprocess.check_call(["g++", "-std=c++17", str(src), "-o", str(exe)])
    size, task, ch, off, by = map(int, subprocess.check_output([str(exe)], text=True).split())
    from importlib import import_module
    snap = import_module("aircombat-selfplay_amd.snapshot")
    assert size == snap.HEADER_BYTES and task == 72 and ch == snap._FIXED.size - 16 and off == snap._FIXED.size
    assert by == off + 8 * snap.MAX_SECTIONS


def test_header_round_trip(pkg):
    from importlib import import_module
    snap = import_module("aircombat-selfplay_amd.snapshot")
    h = header(pkg)
    b = snap.encode_header(h)
    assert len(b) == 1024
    d = snap.decode_header(b)
    for k, v in h.items():
        assert d[k] == v, k
    assert d["magic"] == snap.MAGIC and d["format"] == snap.FORMAT


def blob(pkg, **kw):
    from importlib import import_module
    snap = import_module("aircombat-selfplay_amd.snapshot")
    h = header(pkg, **kw)
    return snap.encode_header(h) + bytes(h["total_bytes"] - 1024)


def test_from_bytes_accepts_its_own(pkg):
    s = pkg.EnvSnapshot.from_bytes(blob(pkg))
    assert not s.on_device and s.E == 4096 and s.nbytes == 4352
    assert s.to_bytes() == blob(pkg)
    assert pkg.EnvSnapshot.from_bytes(s.to_bytes(), expect=s).header == s.header


def test_from_bytes_rejects_mismatches(pkg):
    good = pkg.EnvSnapshot.from_bytes(blob(pkg))
    with pytest.raises(pkg.SnapshotMismatch, match="written by"):
        pkg.EnvSnapshot.from_bytes(blob(pkg, version="aircombat-hip 0.0 (gfx950)"))
    with pytest.raises(pkg.SnapshotMismatch, match="config_hash"):
        pkg.EnvSnapshot.from_bytes(blob(pkg, config_hash=0x0123456789ABCDEE), expect=good)
    with pytest.raises(pkg.SnapshotMismatch, match="E is 2048"):
        pkg.EnvSnapshot.from_bytes(blob(pkg, E=2048), expect=good)
    with pytest.raises(pkg.SnapshotMismatch, match="ctl_precision"):
        pkg.EnvSnapshot.from_bytes(blob(pkg, ctl_precision=1), expect=good.header)
    with pytest.raises(pkg.SnapshotMismatch, match="format"):
        pkg.EnvSnapshot.from_bytes(blob(pkg, format=2))
    with pytest.raises(pkg.SnapshotMismatch, match="magic"):
        pkg.EnvSnapshot.from_bytes(blob(pkg, magic=0x12345678))
    with pytest.raises(pkg.SnapshotMismatch, match="holds"):
        pkg.EnvSnapshot.from_bytes(blob(pkg)[:2000])
    with pytest.raises(pkg.SnapshotMismatch):
        pkg.EnvSnapshot.from_bytes(b"\0" * 100)


def test_multi_snapshot_bytes(pkg):
    one = pkg.EnvSnapshot.from_bytes(blob(pkg))
    m = pkg.MultiSnapshot([one, one], [(0, 4096), (4096, 4096)])
    back = pkg.MultiSnapshot.from_bytes(m.to_bytes())
    assert back.blocks == m.blocks and [p.header for p in back.parts] == [one.header, one.header]
    assert np.array_equal(back.parts[1].data, one.data)
