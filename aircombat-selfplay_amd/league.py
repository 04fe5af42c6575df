"""A round-robin of the members of a ``DevicePolicyPool`` against each other on the device, and its payoff table
(include/aircombat_league.h).

The reference keeps one Elo number per checkpoint, which moves only when that checkpoint is drawn as an opponent of ``latest``
(runner/selfplay_jsbsim_runner.py:136-227), and ``PFSP.choose`` (algorithms/utils/selfplay.py:50-60) samples from those numbers.
``DeviceLeague`` plays every pair the caller deals to the envs at once: the pool's sided assignment (``assign_sides``) puts member
``members2[e][0]`` on agents ``[0, A/2)`` of env e and member ``members2[e][1]`` on agents ``[A/2, A)``, ONE pool launch per step acts
for both sides of every env, the env steps through its usual path (so an attached flight recorder or spawn curriculum keeps working),
and a post-step kernel does the evaluator's bookkeeping over one state array (csrc/league_collect.hpp). ``table()`` reduces the
per-env episode log on the device into a ``LeagueTable``: for every ordered pair (i, j) the episodes, wins / draws / losses, timeouts,
steps and both sides' reward sums, bit-identical from run to run.

Out of scope: ``MultiDeviceVecEnv`` (one league per device) and graph capture.
"""
import ctypes as C

import numpy as np

from .capi import AcLeagueCell, AcLeagueConfig, AcLeagueState
from .policy import HID
from .rollout import device_view, stream_of

_U64 = 2 ** 64 - 1
_CELL = np.dtype([("episodes", "<i8"), ("wins_a", "<i8"), ("wins_b", "<i8"), ("draws", "<i8"), ("timeouts", "<i8"), ("steps", "<i8"),
                  ("sum_a", "<f8"), ("sum_b", "<f8")])
assert _CELL.itemsize == C.sizeof(AcLeagueCell) == 64


def round_robin(E, members, mirror=True, self_play=False):
    """``members2 [E, 2]`` int32 for ``E`` envs: the ordered pairs (i, j) of the member indices ``members`` in lexicographic order
    (i != j unless ``self_play``, which adds the pairs (i, i); without ``mirror`` only i < j of the unequal pairs), dealt to the envs as
    ``np.array_split(np.arange(E), P)`` deals them, range p to pair p, the way ``assign_split`` does. Raises ``ValueError`` when there
    are fewer envs than pairs, or a member is listed twice."""
    ids = sorted(int(m) for m in members)
    if len(set(ids)) != len(ids):
        raise ValueError("round_robin: a member is listed twice")
    pairs = [(i, j) for i in ids for j in ids if (i != j or self_play) and (mirror or i <= j)]
    E = int(E)
    if not pairs:
        raise ValueError("round_robin: no pairs (one member needs self_play=True)")
    if E < len(pairs):
        raise ValueError(f"round_robin: {E} envs cannot hold {len(pairs)} pairs")
    members2 = np.empty((E, 2), dtype=np.int32)
    for p, idx in enumerate(np.array_split(np.arange(E), len(pairs))):
        members2[idx] = pairs[p]
    return members2


class LeagueTable:
    """The payoff table of a league: numpy arrays ``[C, C]`` (C the pool's capacity), cell (i, j) over the logged episodes of the envs
    in which member i flew agents ``[0, A/2)`` (side a) against member j on ``[A/2, A)`` (side b): ``episodes``, ``wins_a``, ``wins_b``,
    ``draws``, ``timeouts``, ``steps`` (int64) and ``sum_a``, ``sum_b`` (float64 sums of the sides' episode rewards, an episode's reward
    being the float32 mean over the side's agents). A win is a reward difference beyond ``win_margin``; exactly the margin is a draw."""

    FIELDS = ("episodes", "wins_a", "wins_b", "draws", "timeouts", "steps", "sum_a", "sum_b")

    def __init__(self, cells, win_margin=100.0):
        cells = np.asarray(cells)
        if cells.dtype != _CELL or cells.ndim != 2 or cells.shape[0] != cells.shape[1]:
            raise ValueError("LeagueTable: cells must be a [C, C] array of ac_league_cell_t records")
        for f in self.FIELDS:
            setattr(self, f, np.ascontiguousarray(cells[f]))
        self.win_margin = float(win_margin)

    def _per_episode(self, total):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.episodes > 0, total / self.episodes, np.nan)

    @property
    def mean_a(self):
        """side a's mean episode reward per cell (NaN without episodes)"""
        return self._per_episode(self.sum_a)

    @property
    def mean_b(self):
        return self._per_episode(self.sum_b)

    @property
    def mean_length(self):
        return self._per_episode(self.steps.astype(np.float64))

    def score(self):
        """``(wins_a + 0.5 draws) / episodes`` per cell: member i's score against member j from side a (NaN without episodes)"""
        return self._per_episode(self.wins_a + 0.5 * self.draws)

    def against(self, i):
        """Row i in the form ``elo_update(latest_elo, opponent_elos, learner_avg, opponent_avg)`` takes: ``(opponents, learner_avg,
        opponent_avg)``, the members j with ``episodes[i, j] > 0`` and the two average episode rewards against each."""
        i = int(i)
        opp = np.nonzero(self.episodes[i] > 0)[0]
        return opp.astype(np.int32), self.mean_a[i, opp], self.mean_b[i, opp]


class DeviceLeague:
    """``DeviceLeague(envs, pool, episodes_per_env=1, deterministic=False, win_margin=100.0)``: ``pool`` (a ``DevicePolicyPool`` of the
    env's observation form) acts for every agent of ``envs`` under a sided assignment, which must be in force for the env's E and A when
    the league is made (``pool.assign_sides(round_robin(E, ids), A)``). Every env logs its first ``episodes_per_env`` episodes. Sampling
    is the default: a deterministic pair from one spawn point repeats the same episode. ``pair(members2)`` deals new pairs, then reset
    the env, ``begin()`` and ``run(n)``, or ``evaluate(max_steps)``; ``table()`` gives the ``LeagueTable``. The handles must stay open
    while the league is. A refusal raises ``ValueError`` and changes nothing."""

    _VIEWS = {"states": ("h", "<f4"), "masks": ("masks", "<f4"), "cum": ("cum", "<f4"), "lengths": ("len", "<i4"), "counts": ("count", "<i4"),
              "log_returns": ("log_ret", "<f4"), "log_lengths": ("log_len", "<i4"), "log_end_steps": ("log_end", "<i4"),
              "log_codes": ("log_code", "<i4"), "members2": ("members2", "<i4"), "remaining": ("remaining", "<i4")}

    def __init__(self, envs, pool, episodes_per_env=1, deterministic=False, win_margin=100.0):
        self.lib = envs.lib
        self.envs, self.pool = envs, pool
        self.episodes_per_env = int(episodes_per_env)
        self.win_margin = float(win_margin)
        self.device_id = int(pool.device_id)
        cfg = AcLeagueConfig(self.episodes_per_env, int(bool(deterministic)), self.win_margin, 0)
        h = C.c_void_p()
        self._h = None
        if self.lib.ac_league_create(envs._h, pool._h, C.byref(cfg), C.byref(h)) != 0:
            raise ValueError(self.lib.last_error())
        self._h = h
        self._last_stream = None
        self._cells = None

    def close(self):
        if getattr(self, "_h", None):
            self.lib.ac_league_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _state(self):
        st = AcLeagueState()
        self.lib.check(self.lib.ac_league_state(self._h, C.byref(st)), "ac_league_state")
        return st

    @property
    def steps(self):
        """steps queued since ``begin`` (-1 before the first ``begin``)"""
        return int(self._state().step)

    def view(self, name):
        """torch view of one of the league's device arrays (it owns them; read them on the stream ``run`` was given, or after a
        synchronize): ``states`` [E * A, 1, 128], ``masks`` [E * A, 1], ``cum`` [E, A], ``lengths`` [E], ``counts`` [E], ``log_returns``
        [E, K, A], ``log_lengths`` / ``log_end_steps`` / ``log_codes`` [E, K], ``members2`` [E, 2] (the pairs as of ``begin``),
        ``remaining`` [1]."""
        field, typestr = self._VIEWS[name]
        st = self._state()
        E, A, K = st.E, st.A, st.K
        shape = {"states": (E * A, 1, HID), "masks": (E * A, 1), "cum": (E, A), "lengths": (E,), "counts": (E,), "log_returns": (E, K, A),
                 "log_lengths": (E, K), "log_end_steps": (E, K), "log_codes": (E, K), "members2": (E, 2), "remaining": (1,)}[name]
        return device_view(getattr(st, field), shape, self.device_id, typestr)

    def pair(self, members2):
        """Deal the pairs ``members2 [E, 2]`` to the envs: ``pool.assign_sides(members2, A, check=True)``. ``begin()`` takes them up."""
        self.pool.assign_sides(members2, self.envs.num_agents, check=True)
        return self

    def begin(self, stream=None):
        """Queue the start of a round: GRU states zero, masks one, running sums and the log cleared, every env with its whole quota to
        go, the pool's pairs copied into the league. One small read-back refuses a side assigned -1 or a member that is not loaded.
        The env is not reset: reset it first."""
        tstream, raw = stream_of(self.device_id, stream)
        if self.lib.ac_league_begin(self._h, raw) != 0:
            raise ValueError(self.lib.last_error())
        self._last_stream = tstream

    def run(self, n_steps, stream=None):
        """Queue ``n_steps`` steps and return without waiting, ordered around ``stream`` as ``DeviceEvaluator.run`` is. Step t draws
        with ``pool.counter + t``; the counter advances by ``n_steps`` (by the steps queued, should the runtime refuse a launch part of
        the way). Returns ``n_steps``."""
        n_steps = int(n_steps)
        tstream, raw = stream_of(self.device_id, stream)
        before = self.steps
        rc = self.lib.ac_league_run(self._h, raw, n_steps, C.c_uint64(self.pool.seed & _U64), C.c_uint64(self.pool.counter & _U64))
        done = n_steps if rc == 0 else max(self.steps - before, 0)
        self.pool.counter += done
        if done:
            self._last_stream = tstream
        if rc != 0:
            raise ValueError(self.lib.last_error())
        return n_steps

    def _stream(self, stream):
        return stream_of(self.device_id, stream)[0] if stream is not None else (self._last_stream or stream_of(self.device_id, None)[0])

    def remaining(self, stream=None):
        """The number of envs that have not finished ``episodes_per_env`` episodes yet: one 4-byte read that waits for ``stream``
        (default: the stream of the last ``begin`` / ``run``)."""
        import torch
        with torch.cuda.stream(self._stream(stream)):
            return int(self.view("remaining").item())

    def evaluate(self, max_steps, chunk=64, stream=None):
        """``begin()``, then ``run(chunk)`` and one read of ``remaining`` in turn (the only host wait, once per chunk) until every env
        has finished its quota or ``max_steps`` steps have run. Returns the ``LeagueTable``."""
        max_steps, chunk = int(max_steps), int(chunk)
        if max_steps < 1 or chunk < 1:
            raise ValueError("evaluate: max_steps and chunk must be at least 1")
        self.begin(stream)
        steps = 0
        while steps < max_steps:
            steps += self.run(min(chunk, max_steps - steps), stream)
            if self.remaining() == 0:
                break
        return self.table()

    def table(self, stream=None):
        """The log so far reduced on the device into a ``LeagueTable`` (two kernels, then one [C, C] x 64-byte copy that waits for
        ``stream``, default the stream of the last ``begin`` / ``run``)."""
        import torch
        s = self._stream(stream)
        Cn = int(self._state().C)
        with torch.cuda.stream(s):
            if self._cells is None or self._cells.numel() != Cn * Cn * 64:
                self._cells = torch.empty(Cn * Cn * 64, dtype=torch.uint8, device=f"cuda:{self.device_id}")
            if self.lib.ac_league_table(self._h, s.cuda_stream, self._cells.data_ptr()) != 0:
                raise ValueError(self.lib.last_error())
            raw = self._cells.cpu().numpy()
        return LeagueTable(raw.view(_CELL).reshape(Cn, Cn).copy(), self.win_margin)


def table_host(log_returns, log_lengths, log_codes, counts, members2, capacity, win_margin, lib=None):
    """``ac_league_table_host``: the device's reduction on host arrays (``log_returns [E, K, A]`` float32, ``log_lengths`` /
    ``log_codes [E, K]``, ``counts [E]``, ``members2 [E, 2]``), as a ``LeagueTable`` of side ``capacity``."""
    from .capi import AcLeagueTableArgs, load_library
    lib = lib or load_library()
    ret = np.ascontiguousarray(log_returns, dtype=np.float32)
    if ret.ndim != 3:
        raise ValueError("table_host: log_returns must be [E, K, A]")
    E, K, A = ret.shape
    ln, code = (np.ascontiguousarray(x, dtype=np.int32) for x in (log_lengths, log_codes))
    cnt, m2 = np.ascontiguousarray(counts, dtype=np.int32), np.ascontiguousarray(members2, dtype=np.int32)
    if ln.shape != (E, K) or code.shape != (E, K) or cnt.shape != (E,) or m2.shape != (E, 2):
        raise ValueError("table_host: log_lengths / log_codes [E, K], counts [E] and members2 [E, 2] must fit log_returns [E, K, A]")
    Cn = int(capacity)
    out = np.zeros((max(Cn, 0), max(Cn, 0)), dtype=_CELL)
    args = AcLeagueTableArgs(E, A, K, Cn, float(win_margin), 0, ret.ctypes.data, ln.ctypes.data, code.ctypes.data, cnt.ctypes.data,
                             m2.ctypes.data, out.ctypes.data)
    if lib.ac_league_table_host(C.byref(args)) != 0:
        raise ValueError(lib.last_error())
    return LeagueTable(out, win_margin)
