"""Spawn curricula on the device (include/aircombat_spawn.h): per-env stages from a bank of reset templates.

``cur = envs.spawn_curriculum(angles=range(181))`` builds the reference's curriculum table (``config.curriculum_bank``: 181 spawns of
the ego team on a circle about the enemy) as a bank of reset templates in device memory and attaches it to a ``HipVecEnv`` /
``HipShareVecEnv``; ``init_states=rows`` takes any ``[K][A]`` spawns instead (``AcInitState`` rows, or dicts with the YAML's ``ic_*``
keys). From then on one small kernel behind every step the handle takes -- on whatever path: ``step``, ``step_device``,
``DeviceRollout.collect``, ``DeviceMAPPORollout.collect``, ``DeviceEvaluator.run`` -- and behind ``reset()`` respawns every env that has
just been reset from the bank entry its stage selects. Until an env's first reset after the attach it keeps flying what it flew.

``mode="fixed"`` leaves the stages to the caller: ``cur.stage`` is a writable int32 torch view in device memory, so a runner can drive
it from ``DeviceEvaluator`` results with torch ops and no host wait. A write takes effect at that env's next reset and never disturbs a
running episode; whatever is written, the device clamps it into the bank. ``mode="auto"`` advances an env's stage on the device when
it has played at least ``window`` episodes at the stage and won ``ceil(win_rate * window)`` of the last ``window``; an episode is won
when the mean return of the ego team reaches ``win_return`` (reward scales differ per task, so there is no default). This restates
the reference's rule rather than copying it: as written there it never fires (config.py, CURRICULUM_BASE).

``sample="at"`` respawns from the stage's own entry, ``sample="upto"`` from a uniform draw among the entries up to it, keyed by
``(seed, env, episode ordinal)`` with the library's counter generator (``draw`` below is the same function on the host).

Views (``stage``, ``spawned``, ``episode``, ``played``, ``wins``, ``return_sum``, ``ret_acc``) are written on the handle's stream: read
them after ``envs.sync()`` or order your stream behind it (``step_device(stream=...)``). While a bank is attached, host steps are
dispatched as HIP launches instead of AQL packets.

Not covered: ``MultiDeviceVecEnv`` (one curriculum per part), snapshots (a snapshot carries no stage; ``restore`` / ``clone_envs`` leave
the curriculum's per-env arrays as they are), per-stage changes to anything but initial conditions, the heading task (it has no reset
template) and graph capture.
"""
import ctypes as C
import math

from .capi import (AcInitState, AcSpawnConfig, AcSpawnState, AC_SPAWN_FIXED, AC_SPAWN_AUTO, AC_SPAWN_AT, AC_SPAWN_UPTO)

MODES = {"fixed": AC_SPAWN_FIXED, "auto": AC_SPAWN_AUTO}
SAMPLES = {"at": AC_SPAWN_AT, "upto": AC_SPAWN_UPTO}
_FIELDS = (("stage", "<i4"), ("spawned", "<i4"), ("episode", "<i4"), ("ret_acc", "<f4"), ("wins", "<i4"), ("played", "<i4"), ("return_sum", "<f4"))


def spawn_config(mode="fixed", sample="at", win_return=None, window=20, win_rate=0.9, seed=0):
    """The keywords of ``spawn_curriculum`` as an ``AcSpawnConfig``: ``min_wins = ceil(win_rate * window)``; the library checks the ranges."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)} (got {mode!r})")
    if sample not in SAMPLES:
        raise ValueError(f"sample must be one of {sorted(SAMPLES)} (got {sample!r})")
    if mode == "auto" and win_return is None:
        raise ValueError("mode='auto' needs win_return: the mean ego return from which an episode counts as won (reward scales differ per task)")
    if not 0.0 < float(win_rate) <= 1.0:
        raise ValueError(f"win_rate must be in (0, 1] (got {win_rate})")
    c = AcSpawnConfig()
    c.mode, c.sample, c.window = MODES[mode], SAMPLES[sample], int(window)
    c.min_wins = int(math.ceil(float(win_rate) * int(window) - 1e-9))
    c.win_return = float("nan") if win_return is None else float(win_return)
    c.seed = int(seed) & (2 ** 64 - 1)
    return c


def pack_rows(rows, num_agents):
    """``[K][A]`` spawns (``AcInitState`` rows or dicts with the YAML's ``ic_*`` keys) as one ctypes array for ``ac_spawn_attach``."""
    from .config import init_state_from_dict
    rows = [list(r) for r in rows]
    for k, r in enumerate(rows):
        if len(r) != num_agents:
            raise ValueError(f"bank entry {k} has {len(r)} aircraft, the handle has {num_agents}")
    flat = (AcInitState * max(1, len(rows) * num_agents))()
    for k, r in enumerate(rows):
        for i, ic in enumerate(r):
            flat[k * num_agents + i] = init_state_from_dict(ic) if isinstance(ic, dict) else AcInitState.from_buffer_copy(ic)
    return flat, len(rows)


def draw(lib, seed, env, episode, stage):
    """``ac_spawn_draw_host``: the ``sample="upto"`` draw of (seed, env, episode ordinal) for a clamped stage, an index in [0, stage]."""
    out = C.c_int32()
    if lib.ac_spawn_draw_host(int(seed) & (2 ** 64 - 1), int(env), int(episode), int(stage), C.byref(out)) != 0:
        raise ValueError(lib.last_error())
    return int(out.value)


class SpawnCurriculum:
    """``SpawnCurriculum(envs, angles=... | init_states=..., mode=, sample=, win_return=, window=, win_rate=, seed=)``: builds the bank and
    attaches it (``HipVecEnv.spawn_curriculum`` does just this). A refusal by the library -- the heading task, a second bank on one
    handle, a bank of no or more than 1024 entries, an entry ``ac_create`` would refuse as an initial condition (the message names it),
    ``window`` outside 1 .. 32, ``min_wins`` outside 1 .. window, an allocation the runtime refuses -- raises ``ValueError`` with the
    library's message and changes nothing."""

    def __init__(self, env, angles=None, init_states=None, mode="fixed", sample="at", win_return=None, window=20, win_rate=0.9, seed=0):
        from .config import curriculum_bank
        self.lib = env.lib
        self._h = None
        self._env = env
        if (angles is None) == (init_states is None):
            raise ValueError("give either angles= (the reference's curriculum table) or init_states= ([K][A] spawns)")
        rows = curriculum_bank(env.config, angles) if init_states is None else init_states
        self.angles = None if angles is None else [int(a) for a in angles]
        flat, K = pack_rows(rows, env.num_agents)
        self._cfg = spawn_config(mode, sample, win_return, window, win_rate, seed)
        h = C.c_void_p()
        if self.lib.ac_spawn_attach(env._h, flat, K, C.byref(self._cfg), C.byref(h)) != 0:
            raise ValueError(self.lib.last_error())
        self._h = h
        st = AcSpawnState()
        if self.lib.ac_spawn_state(self._h, C.byref(st)) != 0:
            raise ValueError(self.lib.last_error())
        self.num_entries, self.num_envs, self.device_id = int(st.K), int(st.E), env._device_id
        self._ptrs = {n: getattr(st, n) for n, _ in _FIELDS}
        self._views = {}
        env._curriculum = self

    @property
    def attached(self):
        return self._h is not None

    def _view(self, name):
        if self._h is None:
            raise ValueError("the curriculum has been detached: its per-env arrays are gone")
        if name not in self._views:
            from .rollout import device_view
            self._views[name] = device_view(self._ptrs[name], (self.num_envs,), self.device_id, dict(_FIELDS)[name])
        return self._views[name]

    stage = property(lambda self: self._view("stage"), doc="int32 [E], writable: the bank entry (or, with sample='upto', the highest one) of each env's next respawn")
    spawned = property(lambda self: self._view("spawned"), doc="int32 [E]: the bank entry each env's running episode was spawned from (-1: the handle's own template)")
    episode = property(lambda self: self._view("episode"), doc="int32 [E]: ordinal of each env's running episode, counted from the attach")
    ret_acc = property(lambda self: self._view("ret_acc"), doc="float32 [E]: mean ego return of the running episode so far")
    wins = property(lambda self: self._view("wins"), doc="int32 [E]: shift register of win bits, the latest episode in bit 0")
    played = property(lambda self: self._view("played"), doc="int32 [E]: episodes scored at the env's stage")
    return_sum = property(lambda self: self._view("return_sum"), doc="float32 [E]: sum of their returns")

    def histogram(self):
        """Envs per stage (stages clamped into the bank as the device clamps them), a list of ``num_entries`` counts; one read, after
        waiting for the handle's stream."""
        import torch
        self._env.sync()
        st = self.stage.clamp(0, self.num_entries - 1).to(torch.int64)
        return torch.bincount(st, minlength=self.num_entries).tolist()

    def set_config(self, mode="fixed", sample="at", win_return=None, window=20, win_rate=0.9, seed=0):
        """Change the mode, rule and sampling from the next step on; the per-env arrays stay as they are."""
        if self._h is None:
            raise ValueError("the curriculum has been detached")
        cfg = spawn_config(mode, sample, win_return, window, win_rate, seed)
        if self.lib.ac_spawn_set_config(self._h, C.byref(cfg)) != 0:
            raise ValueError(self.lib.last_error())
        self._cfg = cfg

    def close(self):
        """Detach from the handle and free the bank (``HipVecEnv.stop_curriculum``); the views are gone with it."""
        if getattr(self, "_h", None) is not None:
            self._views, self._h = {}, None
            env = self._env
            if getattr(env, "_curriculum", None) is self:
                env._curriculum = None
                if not env.closed:
                    env.lib.check(env.lib.ac_spawn_detach(env._h), "ac_spawn_detach")
