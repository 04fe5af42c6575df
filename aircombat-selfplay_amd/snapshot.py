"""EnvSnapshot: the whole state of a HipVecEnv's envs as a value (include/aircombat.h, ac_snapshot_*).

A snapshot is a 1024-byte header followed by the device arrays of every env (csrc/snapshot.hpp). It lives in device memory (a torch
uint8 tensor on the env's GPU) or in host memory (a numpy uint8 array), and ``to_bytes()`` / ``EnvSnapshot.from_bytes()`` carry it
through a ``torch.save`` checkpoint. The header is decoded here without a GPU, so a checkpoint can be checked before any env exists.
"""
import struct

import numpy as np

MAGIC = 0x4E534341          # "ACSN"
FORMAT = 1
HEADER_BYTES = 1024
MAX_SECTIONS = 32
_FIXED = struct.Struct("<II64s12iQQ")          # magic, format, version, 12 int32 fields, config_hash, total_bytes
_INTS = ("task", "E", "A", "msl_slots", "obs_dim", "act_dim", "act_low", "ctl_precision", "hierarchical", "n_sections", "reserved0", "reserved1")
# the fields two snapshots (or a snapshot and a handle) must share for one to load into the other
IDENTITY = ("version", "task", "E", "A", "msl_slots", "obs_dim", "act_dim", "act_low", "ctl_precision", "hierarchical", "config_hash",
            "total_bytes", "n_sections")


class SnapshotMismatch(ValueError):
    """A snapshot that does not fit the env (or the library) it is offered to."""


def encode_header(h):
    """dict (decode_header's keys) -> the 1024 header bytes."""
    ints = [int(h.get(k, 0)) for k in _INTS]
    out = bytearray(HEADER_BYTES)
    _FIXED.pack_into(out, 0, int(h.get("magic", MAGIC)), int(h.get("format", FORMAT)), h["version"].encode()[:63], *ints,
                     int(h["config_hash"]), int(h["total_bytes"]))
    off, size = list(h.get("offsets", [])), list(h.get("bytes", []))
    off += [0] * (MAX_SECTIONS - len(off))
    size += [0] * (MAX_SECTIONS - len(size))
    struct.pack_into(f"<{MAX_SECTIONS}Q{MAX_SECTIONS}Q", out, _FIXED.size, *off, *size)
    return bytes(out)


def decode_header(b):
    """The first 1024 bytes of a snapshot -> dict; SnapshotMismatch when they are not a snapshot header of this format."""
    b = bytes(memoryview(b)[:HEADER_BYTES])
    if len(b) < HEADER_BYTES:
        raise SnapshotMismatch(f"a snapshot starts with a {HEADER_BYTES}-byte header; got {len(b)} bytes")
    v = _FIXED.unpack_from(b, 0)
    h = {"magic": v[0], "format": v[1], "version": v[2].split(b"\0", 1)[0].decode(errors="replace")}
    h.update(zip(_INTS, v[3:3 + len(_INTS)]))
    h["config_hash"], h["total_bytes"] = v[-2], v[-1]
    s = struct.unpack_from(f"<{MAX_SECTIONS}Q{MAX_SECTIONS}Q", b, _FIXED.size)
    n = max(0, min(h["n_sections"], MAX_SECTIONS))
    h["offsets"], h["bytes"] = list(s[:n]), list(s[MAX_SECTIONS:MAX_SECTIONS + n])
    if h["magic"] != MAGIC:
        raise SnapshotMismatch("not an env snapshot (bad magic word)")
    if h["format"] != FORMAT:
        raise SnapshotMismatch(f"snapshot format {h['format']}, this library reads format {FORMAT}")
    return h


def check_compatible(got, want, who="snapshot"):
    """Raise SnapshotMismatch naming the first IDENTITY field in which header `got` differs from header `want`."""
    for k in IDENTITY:
        if got.get(k) != want.get(k):
            raise SnapshotMismatch(f"{who}: {k} is {got.get(k)!r}, expected {want.get(k)!r}")


class EnvSnapshot:
    """Opaque state of every env of one handle. ``header`` is the decoded header (task, E, A, config_hash, ...); ``data`` is a torch
    uint8 tensor on the GPU (``device=True`` snapshots) or a numpy uint8 array in host memory. ACMI recording state is not part of it."""

    def __init__(self, header, data, ready=None):
        self.header = header
        self.data = data
        self.ready = ready      # device snapshots: a torch.cuda.Event recorded on the saving handle's stream after the save's copies

    def wait(self):
        """Block until a device snapshot's copies have finished (no-op for host snapshots)."""
        if self.ready is not None:
            self.ready.synchronize()
            self.ready = None

    def __del__(self):
        try:
            self.wait()      # (the save may still be writing the buffer that is about to go back to the allocator)
        except Exception:    # interpreter shutdown
            pass

    on_device = property(lambda self: not isinstance(self.data, np.ndarray))
    nbytes = property(lambda self: int(self.header["total_bytes"]))

    def __getattr__(self, name):      # header fields as attributes: snap.E, snap.task, snap.config_hash, ...
        h = self.__dict__.get("header")
        if h is not None and name in h:
            return h[name]
        raise AttributeError(name)

    def to_host(self):
        """The same snapshot in host memory (a copy if it is on the device)."""
        if not self.on_device:
            return self
        self.wait()       # (the save's copies run on the handle's stream, .cpu() on torch's)
        return EnvSnapshot(self.header, self.data.cpu().numpy())

    def to_bytes(self):
        """The snapshot as bytes (header included): what EnvSnapshot.from_bytes takes back, e.g. out of a torch.save checkpoint."""
        return self.to_host().data.tobytes()

    @classmethod
    def from_bytes(cls, b, expect=None, lib=None):
        """A host snapshot from bytes. Checks the header: magic word, format, the size, the writing library's ac_version() against
        the loaded library's (``lib``, default: the package's), and with ``expect`` (an EnvSnapshot, a header dict or an env with
        ``snapshot_header()``) every identity field, the config digest included. SnapshotMismatch on any difference."""
        h = decode_header(b)
        if len(b) < h["total_bytes"]:
            raise SnapshotMismatch(f"snapshot holds {h['total_bytes']} bytes, got {len(b)}")
        if lib is None:
            from .capi import load_library
            lib = load_library()
        version = lib.ac_version().decode()
        if h["version"] != version:
            raise SnapshotMismatch(f"snapshot written by {h['version']!r}, this library is {version!r}")
        if expect is not None:
            want = expect.header if isinstance(expect, EnvSnapshot) else (expect if isinstance(expect, dict) else expect.snapshot_header())
            check_compatible(h, want, "EnvSnapshot.from_bytes")
        data = np.frombuffer(b, dtype=np.uint8, count=h["total_bytes"]).copy()
        return cls(h, data)

    def __repr__(self):
        h = self.header
        return f"EnvSnapshot(task={h['task']}, E={h['E']}, A={h['A']}, {self.nbytes} bytes, {'device' if self.on_device else 'host'})"


class MultiSnapshot:
    """MultiDeviceVecEnv.snapshot(): one EnvSnapshot per part, with the env block (start, count) each part holds."""

    def __init__(self, parts, blocks):
        self.parts, self.blocks = list(parts), [tuple(b) for b in blocks]

    _MULTI = struct.Struct("<IIqqQ")    # per part: magic, part index, env block start, env block count, snapshot bytes

    def to_bytes(self):
        out = []
        for i, (p, (start, count)) in enumerate(zip(self.parts, self.blocks)):
            b = p.to_bytes()
            out += [self._MULTI.pack(MAGIC, i, start, count, len(b)), b]
        return b"".join(out)

    @classmethod
    def from_bytes(cls, b, lib=None):
        parts, blocks, pos = [], [], 0
        while pos < len(b):
            magic, i, start, count, n = cls._MULTI.unpack_from(b, pos)
            if magic != MAGIC or i != len(parts):
                raise SnapshotMismatch("not a multi-device snapshot")
            pos += cls._MULTI.size
            parts.append(EnvSnapshot.from_bytes(b[pos:pos + n], lib=lib))
            blocks.append((start, count))
            pos += n
        return cls(parts, blocks)
