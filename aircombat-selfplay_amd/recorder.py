"""The device flight recorder (include/aircombat_record.h): ACMI recordings of any env from episodes that ran on the device.

``rec = envs.record(envs=[...], frames=F)`` attaches a ``FlightRecorder`` to a ``HipVecEnv`` / ``HipShareVecEnv``. From then on one
small kernel behind every step the handle takes -- on whatever path: ``step``, ``step_device``, ``DeviceRollout.collect``,
``DeviceMAPPORollout.collect``, ``DeviceEvaluator.run`` -- and behind ``reset()`` appends what BaseEnv.render reads (env_base.py:207-250)
for the chosen envs to a ring of ``F`` frames in device memory: the step counter, every aircraft's entity values and status, its
munition slots and the scenario tasks' packed extension words. Afterwards ``frames(env)`` pulls one env's frames, ``episodes(env)``
finds the episodes among them and ``write_acmi(path, env, first, last)`` writes the file ``render()`` would have written had it been
called after each of those steps, byte for byte: both feed ``acmi.FrameWriter``. Which env and which episode is decided after the
fact. A handle with a recorder attached takes its host steps through HIP launches instead of the AQL queue.

Frame ``f`` lives in ring slot ``f % F``; frames ``[max(0, count - F), count)`` are readable. The column table comes from
``ac_recorder_layout``; no offset is written down here.

Not covered: a terminal-state frame taken before the auto-reset (the frame of the step that ended an episode already shows the next
one, as ``render()`` does), ``MultiDeviceVecEnv`` (one recorder per part), ``restore()`` / ``clone_envs`` (the recorder does not
follow them: a restored handle simply records what it steps through next), binary ACMI and graph capture.
"""
import ctypes as C
import weakref

import numpy as np

from . import acmi
from .capi import AcRecorderInfo, AcRecorderLayout


def layout(lib, task, num_agents, msl_slots, has_ext):
    """``ac_recorder_layout`` as (columns, bytes per aircraft-frame): columns is a list of (name, numpy typestr, elements per aircraft)."""
    out = AcRecorderLayout()
    if lib.ac_recorder_layout(int(task), int(num_agents), int(msl_slots), int(bool(has_ext)), C.byref(out)) != 0:
        raise ValueError(lib.last_error())
    cols = [(out.columns[i].name.decode(), {4: "<i4", 8: "<f8"}[out.columns[i].elem_size], int(out.columns[i].count)) for i in range(out.n_columns)]
    return cols, int(out.bytes_per_aircraft_frame)


def frame_dtype(columns):
    """The packed numpy record of one aircraft-frame. ``msl_pose`` is [slot][px, py, pz, theta, psi]; the per-slot columns are [slot]."""
    fields = []
    for name, typestr, count in columns:
        shape = (count // 5, 5) if name == "msl_pose" else ((count,) if count > 1 else ())
        fields.append((name, typestr, shape) if shape else (name, typestr))
    return np.dtype(fields)


def ring_slot(f, capacity):
    """ring slot of frame f"""
    return int(f) % int(capacity)


def readable_range(count, capacity):
    """(first, end): frames [first, end) are in the ring after `count` captures"""
    return max(0, int(count) - int(capacity)), int(count)


def check_span(count, capacity, first, last):
    """Frames [first, last] of a ring that has taken `count` captures: returns (first, n), or raises ValueError for a span that is empty,
    has been overwritten or has not been captured."""
    lo, hi = readable_range(count, capacity)
    first, last = int(first), int(last)
    if last < first:
        raise ValueError(f"frames {first} .. {last}: an empty span")
    if first < lo:
        raise ValueError(f"frame {first} has been overwritten (readable: {lo} .. {hi - 1})")
    if last >= hi:
        raise ValueError(f"frame {last} has not been captured (readable: {lo} .. {hi - 1})")
    return first, last - first + 1


def episode_spans(cur_steps, first_frame=0):
    """Episodes among consecutive frames whose step counters are ``cur_steps``, the first of them frame ``first_frame``: a new span
    starts wherever the counter does not increase (a reset, or the auto-reset inside the step that ended an episode). Returns
    [(first, last), ...] in frame indices, both ends included. The first span may be the tail of an episode whose start has left the
    ring, and the last may still be running."""
    steps = [int(v) for v in cur_steps]
    spans, start = [], 0
    for i in range(1, len(steps) + 1):
        if i == len(steps) or steps[i] <= steps[i - 1]:
            spans.append((first_frame + start, first_frame + i - 1))
            start = i
    return spans


def acmi_text(cfg, frames):
    """The ACMI file of recorded frames (a ``FlightRecorder.frames`` array, [n, A]) as ``render()`` writes it: header, then one frame per row."""
    w = acmi.FrameWriter(cfg, frames.shape[1])
    names = frames.dtype.names
    parts = [acmi.HEADER]
    for row in frames:
        A = len(row)
        slots = chaff = None
        if "msl_status" in names:
            slots = [[(row["msl_status"][a][k], row["msl_model"][a][k]) + tuple(row["msl_pose"][a][k]) for k in range(row["msl_status"].shape[1])]
                     for a in range(A)]
        else:
            slots = [[] for _ in range(A)]
        if "ext" in names:
            chaff = [acmi.chaff_from_words(*row["ext"][a]) for a in range(A)]
        parts.append(w.frame(row["cur_step"][0], [row["entity"][a] for a in range(A)], slots, chaff))
    return "".join(parts)


class FlightRecorder:
    """``FlightRecorder(envs, envs=None | indices, frames=F)``: a recorder for a handle, not attached (``capture()`` takes frames
    explicitly); ``HipVecEnv.record`` creates and attaches one. A refusal by the library -- a selection that is unsorted, repeats an env
    or leaves ``[0, E)``, ``frames < 1``, an allocation the runtime refuses, a second recorder attached to one handle, an env that is not
    recorded, frames that have left the ring -- raises ``ValueError`` with the library's message and changes nothing."""

    def __init__(self, env, envs=None, frames=1024):
        self.lib = env.lib
        self._h = None
        self._env = env
        if envs is None:
            self.envs, sel, S = list(range(env.num_envs)), None, env.num_envs
        else:
            self.envs = [int(e) for e in envs]
            S = len(self.envs)
            sel = (C.c_int32 * max(S, 1))(*self.envs)
        h = C.c_void_p()
        if self.lib.ac_recorder_create(env._h, sel, S, int(frames), C.byref(h)) != 0:
            raise ValueError(self.lib.last_error())
        self._h = h
        info = self._info()
        self.capacity, self.num_agents, self.device_id = int(info.F), int(info.A), env._device_id
        self.columns, self.bytes_per_aircraft_frame = layout(self.lib, info.task, info.A, info.msl_slots, info.has_ext)
        self.dtype = frame_dtype(self.columns)
        assert self.dtype.itemsize == self.bytes_per_aircraft_frame
        self.nbytes = int(info.bytes)
        if not hasattr(env, "_recorders"):
            env._recorders = []
        env._recorders.append(weakref.ref(self))     # HipVecEnv.close() closes the recorders made for it

    def _info(self):
        info = AcRecorderInfo()
        if self.lib.ac_recorder_info(self._h, C.byref(info)) != 0:
            raise ValueError(self.lib.last_error())
        return info

    def attach(self, env=None):
        """Attach to the handle the recorder was made for (``env``, if given, must be that handle: the library refuses another)."""
        env = self._env if env is None else env
        if self.lib.ac_recorder_attach(env._h, self._h) != 0:
            raise ValueError(self.lib.last_error())
        env._recorder = self

    @property
    def attached(self):
        return bool(self._info().attached)

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self._env, "_recorder", None) is self:
                self._env._recorder = None
            self.lib.ac_recorder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def count(self):
        """frames captured so far"""
        return int(self.lib.ac_recorder_count(self._h))

    def capture(self, after_reset=False):
        """Queue one frame of the handle's state as it is on its stream now (the attached recorder gets its frames by itself)."""
        if self.lib.ac_recorder_capture(self._h, int(bool(after_reset))) != 0:
            raise ValueError(self.lib.last_error())

    def _span(self, first, last):
        lo, hi = readable_range(self.count, self.capacity)
        return check_span(self.count, self.capacity, lo if first is None else first, hi - 1 if last is None else last)

    def frames(self, env, first=None, last=None):
        """Frames ``first .. last`` (both included; default: everything readable) of recorded env ``env`` as a structured array
        ``[n, A]`` with the layout's columns as fields. One extract kernel and one copy; waits for the handle's stream."""
        if int(env) not in self.envs:
            raise ValueError(f"env {int(env)} is not among the recorded envs")
        f0, n = self._span(first, last)
        A = self.num_agents
        raw = np.empty(n * A * self.bytes_per_aircraft_frame, dtype=np.uint8)
        if self.lib.ac_recorder_read(self._h, int(env), f0, n, raw.ctypes.data) != 0:
            raise ValueError(self.lib.last_error())
        out = np.empty((n, A), dtype=self.dtype)
        off = 0
        for name, typestr, count in self.columns:      # column after column, each [n][count][A]
            size = n * count * A * int(typestr[2:])
            col = raw[off:off + size].view(typestr).reshape(n, count, A).transpose(0, 2, 1)
            out[name] = col.reshape((n, A) + self.dtype[name].shape)
            off += size
        return out

    def view(self, column):
        """torch view (no copy) of one column of the ring, ``[F, count, S, A]``: slot ``f % F`` holds frame f. Captures are written on
        the handle's stream; read after ``envs.sync()`` or order your stream behind it."""
        from .rollout import device_view
        names = [c[0] for c in self.columns]
        i = names.index(column) if isinstance(column, str) else int(column)
        ptr, n = C.c_void_p(), C.c_int64()
        if self.lib.ac_recorder_device_ptr(self._h, i, C.byref(ptr), C.byref(n)) != 0:
            raise ValueError(self.lib.last_error())
        _, typestr, count = self.columns[i]
        shape = (self.capacity, count, len(self.envs), self.num_agents)
        assert int(np.prod(shape)) == n.value
        return device_view(ptr.value, shape, self.device_id, typestr)

    def episodes(self, env):
        """[(first, last), ...]: the episodes of env ``env`` among the readable frames, delimited where ``cur_step`` does not increase."""
        lo, hi = readable_range(self.count, self.capacity)
        if hi == lo:
            return []
        return episode_spans(self.frames(env)["cur_step"][:, 0], lo)

    def write_acmi(self, path, env, first=None, last=None):
        """Write frames ``first .. last`` of env ``env`` as the Tacview file ``render(filepath=path, env=env)`` writes when it is called
        after each of those steps. Returns the number of frames written."""
        fr = self.frames(env, first, last)
        with open(path, mode="w", encoding="utf-8-sig") as f:
            f.write(acmi_text(self._env.config, fr))
        return len(fr)
