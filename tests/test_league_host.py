"""The device league without a GPU (include/aircombat_league.h): the sided plan through the plan's host twin, the post-step kernel's
work-item function (ac_league_post_step_host, csrc/league_collect.hpp) against a numpy restatement of the evaluator's bookkeeping over
one state array plus the done code, the payoff table's host twin (ac_league_table_host) against a numpy loop written in the contract's
two-level summation order, round_robin, the header against its ctypes mirror, and every refusal that returns before touching a device.
All comparisons are bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from league_util import TIMEOUT, assert_table, table_loop, threshold_log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HID = 128


def ptr(a):
    return a.ctypes.data


# ---- exports and the header
LEAGUE_SYMBOLS = {"ac_league_create", "ac_league_destroy", "ac_league_begin", "ac_league_run", "ac_league_state", "ac_league_post_step_host",
                  "ac_league_table", "ac_league_table_host"}


def test_header_bindings_and_exports_agree(pkg, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "aircombat_league.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %d", sizeof(ac_league_config_t), sizeof(ac_league_state_t), '
                   'sizeof(ac_league_post_step_t), sizeof(ac_league_cell_t), sizeof(ac_league_table_args_t), (int)AC_LEAGUE_MAX_EPISODES);'
                   'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a, b, c, d, e, k = map(int, subprocess.check_output([str(exe)], text=True).split())
    capi = pkg.capi
    assert a == C.sizeof(capi.AcLeagueConfig) == 16 and b == C.sizeof(capi.AcLeagueState) and c == C.sizeof(capi.AcLeaguePostStep)
    assert d == C.sizeof(capi.AcLeagueCell) == 64 and e == C.sizeof(capi.AcLeagueTableArgs)
    assert k == capi.AC_LEAGUE_MAX_EPISODES == 64 and capi.AC_DONE_TIMEOUT == TIMEOUT
    hdr = open(os.path.join(ROOT, "include", "aircombat_league.h")).read()
    assert set(re.findall(r"\b(ac_league_[a-z0-9_]+)\s*\(", hdr)) == LEAGUE_SYMBOLS
    assert re.search(r"\bac_policy_pool_assign_sides\s*\(", open(os.path.join(ROOT, "include", "aircombat.h")).read())
    lib = pkg.load_library()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib.path], text=True)
    for sym in LEAGUE_SYMBOLS | {"ac_policy_pool_assign_sides"}:
        assert sym in capi.SIGNATURES and hasattr(lib, sym) and re.search(rf"\bT {sym}\b", exported), sym
    assert set(re.findall(r"\bT (ac_league_[a-z0-9_]+)\b", exported)) == LEAGUE_SYMBOLS
    for name in ("DeviceLeague", "LeagueTable", "round_robin"):
        assert getattr(pkg, name).__name__ == name and name in pkg.__all__
    assert hasattr(pkg.DevicePolicyPool, "assign_sides")


def test_null_handles_are_refused_without_a_device(pkg):
    lib = pkg.load_library()
    out = C.c_void_p()
    assert lib.ac_league_create(None, None, None, C.byref(out)) == -1 and "null argument" in lib.last_error()
    assert lib.ac_league_begin(None, None) == -1 and "null handle" in lib.last_error()
    assert lib.ac_league_run(None, None, 1, 0, 0) == -1 and "null handle" in lib.last_error()
    assert lib.ac_league_state(None, None) == -1
    assert lib.ac_league_table(None, None, None) == -1 and "null argument" in lib.last_error()
    assert lib.ac_league_post_step_host(None) == -1 and lib.ac_league_table_host(None) == -1
    assert lib.ac_league_destroy(None) == 0
    m2 = np.zeros((4, 2), dtype=np.int32)
    assert lib.ac_policy_pool_assign_sides(None, None, ptr(m2), 4, 2) == -1 and "null argument" in lib.last_error()


# ---- the sided plan is the plan over 2 E half-envs of A / 2 rows
@pytest.mark.parametrize("E,A,cap", [(56, 2, 3), (20, 4, 3), (7, 8, 5), (1, 2, 1)])
def test_sided_plan_through_the_plan_host_twin(pkg, E, A, cap):
    plan_host = pkg.policy.plan_host
    rng = np.random.default_rng(E * 100 + A)
    m2 = rng.integers(0, cap, size=(E, 2)).astype(np.int32)
    if E > 3:
        m2[1, 0] = -1          # a side that is not acted for
        m2[3] = (-1, -1)
    loaded = np.ones(cap, dtype=np.int32)
    order, tiles, bad = plan_host(m2.ravel(), A // 2, cap, loaded)
    assert bad == -1
    half = A // 2
    want = {(e * A + a): int(m2[e, a // half]) for e in range(E) for a in range(A) if m2[e, a // half] >= 0}
    seen = {}
    for m, p0, p1 in tiles:
        assert 0 < p1 - p0 <= 32
        for r in order[p0:p1]:
            assert int(r) not in seen
            seen[int(r)] = int(m)
    assert seen == want                      # every call row e * A + a once, under its side's member; rows of a -1 side absent
    assert list(tiles[:, 0]) == sorted(tiles[:, 0])
    mt = C.c_int64()
    assert pkg.load_library().ac_policy_pool_max_tiles(2 * E, half, cap, C.byref(mt)) == 0 and len(tiles) <= mt.value
    # the first bad unit is a half-env: env = unit // 2
    if E > 3:
        m2[2, 1] = cap + 4
        assert plan_host(m2.ravel(), half, cap, loaded)[2] // 2 == 2
        m2[2, 1] = 0
        loaded[m2[0, 0]] = 0
        assert plan_host(m2.ravel(), half, cap, loaded)[2] // 2 == 0


# ---- the post-step body against a numpy restatement
class Book:
    """The evaluator's bookkeeping (header comment of aircombat_eval.h) over one [E * A] state array, plus the done code of the ending
    step, restated in numpy."""

    def __init__(self, E, A, K, h):
        self.E, self.A, self.K = E, A, K
        self.h, self.masks = h.copy(), np.ones(E * A, dtype=np.float32)
        self.cum = np.zeros((E, A), dtype=np.float32)
        self.len, self.count = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.int32)
        self.log_ret = np.zeros((E, K, A), dtype=np.float32)
        self.log_len, self.log_end, self.log_code = (np.zeros((E, K), dtype=np.int32) for _ in range(3))
        self.remaining = np.array([E], dtype=np.int32)

    def step(self, t, rewards, dones, info):
        done_env = dones.reshape(self.E, self.A).all(axis=1)
        self.cum = (self.cum + rewards).astype(np.float32)
        self.len += 1
        for e in np.nonzero(done_env)[0]:
            n = self.count[e]
            if n < self.K:
                self.log_ret[e, n], self.log_len[e, n], self.log_end[e, n], self.log_code[e, n] = self.cum[e], self.len[e], t, info[e, 1]
                if n == self.K - 1:
                    self.remaining[0] -= 1
            self.count[e] += 1
            self.cum[e], self.len[e] = 0.0, 0
            self.h[e * self.A:(e + 1) * self.A] = 0.0
        self.masks = np.repeat(1.0 - done_env.astype(np.float32), self.A)

    def arrays(self):
        return {k: np.array(getattr(self, k)) for k in ("h", "masks", "cum", "len", "count", "log_ret", "log_len", "log_end", "log_code", "remaining")}


def test_post_step_matches_the_restated_bookkeeping(pkg):
    lib, capi = pkg.load_library(), pkg.capi
    E, A, K, T = 5, 4, 2, 6
    # the steps at which each env ends: env 0 three times (the third counted, not logged); envs 1 and 4 fill their second slot on the
    # last step, which is where remaining reaches 0
    ends = {0: [0, 2, 4], 1: [2, 5], 2: [1, 3], 3: [3, 4], 4: [0, 5]}
    rng = np.random.default_rng(7)
    h0 = rng.standard_normal((E * A, HID)).astype(np.float32)
    book = Book(E, A, K, h0)
    dev = Book(E, A, K, h0)
    remaining_seen = []
    for t in range(T):
        rewards = rng.standard_normal((E, A)).astype(np.float32) * 50
        dones = np.zeros((E, A), dtype=np.uint8)
        dones[2, 1] = 1                                # a single agent done while its env goes on
        info = np.zeros((E, 4), dtype=np.int32)
        info[:, 0] = t
        info[:, 1] = 1 + (np.arange(E) + t) % 8        # a code on every step: only the ending step's may be logged
        for e, ts in ends.items():
            if t in ts:
                dones[e] = 1
        h_step = rng.standard_normal((E * A, HID)).astype(np.float32)   # what the policy launch left in the states
        book.h, dev.h = h_step.copy(), h_step.copy()
        book.step(t, rewards, dones, info)
        p = capi.AcLeaguePostStep(E, A, HID, K, t, 0, ptr(rewards), ptr(dones), ptr(info), ptr(dev.h), ptr(dev.masks), ptr(dev.cum), ptr(dev.len),
                                  ptr(dev.count), ptr(dev.log_ret), ptr(dev.log_len), ptr(dev.log_end), ptr(dev.log_code), ptr(dev.remaining))
        assert lib.ac_league_post_step_host(C.byref(p)) == 0, lib.last_error()
        got, want = dev.arrays(), book.arrays()
        for k in want:
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (t, k)
        remaining_seen.append(int(dev.remaining[0]))
    assert list(dev.count) == [3, 2, 2, 2, 2] and remaining_seen[-2] > 0 and remaining_seen[-1] == 0
    assert dev.log_end[0].tolist() == [0, 2] and dev.log_end[1].tolist() == [2, 5]
    assert dev.log_code[1, 1] == 1 + (1 + 5) % 8 and dev.log_code[0, 1] == 1 + (0 + 2) % 8
    assert (dev.h[:A] != 0).all() and (dev.h[A:2 * A] == 0).all()      # env 0 went on at the last step, env 1 ended


def test_post_step_refusals(pkg):
    lib, capi = pkg.load_library(), pkg.capi
    E, A, K = 2, 2, 1
    f = lambda *s: np.zeros(s, dtype=np.float32)
    i = lambda *s: np.zeros(s, dtype=np.int32)
    keep = [f(E, A), np.zeros((E, A), dtype=np.uint8), i(E, 4), f(E * A, HID), f(E * A), f(E, A), i(E), i(E), f(E, K, A), i(E, K), i(E, K), i(E, K), i(1)]
    ok = [E, A, HID, K, 0, 0] + [ptr(a) for a in keep]
    assert lib.ac_league_post_step_host(C.byref(capi.AcLeaguePostStep(*ok))) == 0
    for idx, val, what in [(1, 3, "even A"), (1, 10, "even A"), (0, 0, "E >= 1"), (2, 6, "hidden"), (3, 0, "K must be"), (3, 65, "K must be"),
                           (4, -1, "step"), (8, None, "null array"), (17, None, "null array")]:
        bad = list(ok)
        bad[idx] = val
        assert lib.ac_league_post_step_host(C.byref(capi.AcLeaguePostStep(*bad))) == -1
        assert what in lib.last_error(), (what, lib.last_error())


# ---- the table
@pytest.mark.parametrize("A", [2, 4])
def test_table_host_thresholds_order_and_empty_cells(pkg, A):
    table_host = pkg.league.table_host
    E, K, Cn, margin = 23, 3, 3, 100.0
    log_ret, log_len, log_code, count = threshold_log(E, K, A, margin)
    m2 = np.zeros((E, 2), dtype=np.int32)
    # cells whose envs are not adjacent; cell (2, 1) and the diagonal stay empty; env 7.. cycle over the others
    cycle = [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2)]
    for e in range(E):
        m2[e] = cycle[e % len(cycle)]
    m2[:7] = (0, 1)                             # the threshold episodes all in one cell
    tab = table_host(log_ret, log_len, log_code, count, m2, Cn, margin)
    want = table_loop(log_ret, log_len, log_code, count, m2, Cn, margin)
    assert_table(tab, want)
    assert tab.episodes[2, 1] == 0 and tab.sum_a[2, 1] == 0 and tab.steps[2, 1] == 0 and np.isnan(tab.mean_a[2, 1]) and np.isnan(tab.score()[2, 1])
    assert tab.episodes.sum() == np.minimum(count, K).sum()
    assert (tab.wins_a + tab.wins_b + tab.draws == tab.episodes).all()
    # the seven threshold episodes alone: exactly +-margin and everything inside are draws, the next float32 beyond each is a win
    one = np.zeros(E, dtype=np.int32)
    one[:7] = 1
    t7 = table_host(log_ret, log_len, log_code, one, m2, Cn, margin)
    assert (t7.episodes[0, 1], t7.wins_a[0, 1], t7.wins_b[0, 1], t7.draws[0, 1]) == (7, 1, 1, 5)
    assert t7.score()[0, 1] == (1 + 2.5) / 7
    # margin 0: any difference wins, equality draws
    t0 = table_host(log_ret, log_len, log_code, one, m2, Cn, 0.0)
    assert (t0.wins_a[0, 1], t0.wins_b[0, 1], t0.draws[0, 1]) == (3, 3, 1)
    assert t7.timeouts[0, 1] == int((log_code[:7, 0] == TIMEOUT).sum()) and t7.steps[0, 1] == int(log_len[:7, 0].sum())


def test_table_host_refusals(pkg):
    table_host = pkg.league.table_host
    z = lambda E=2, K=1, A=2: (np.zeros((E, K, A), np.float32), np.zeros((E, K), np.int32), np.zeros((E, K), np.int32), np.zeros(E, np.int32),
                                np.zeros((E, 2), np.int32))
    lib = pkg.load_library()
    for kw, margin, cap, what in [(dict(A=3), 1.0, 2, "even A"), (dict(K=65), 1.0, 2, "K must be"), ({}, -1.0, 2, "win_margin"),
                                  ({}, float("nan"), 2, "win_margin"), ({}, float("inf"), 2, "win_margin"), ({}, 1.0, 0, "C must be")]:
        with pytest.raises(ValueError, match=what):
            table_host(*z(**kw), cap, margin)
    args = pkg.capi.AcLeagueTableArgs(2, 2, 1, 2, 1.0, 0, None, None, None, None, None, None)
    assert lib.ac_league_table_host(C.byref(args)) == -1 and "null array" in lib.last_error()


def test_league_table_views_and_against(pkg):
    table_host = pkg.league.table_host
    E, K, A = 6, 1, 2
    log_ret = np.zeros((E, K, A), np.float32)
    log_ret[:, 0, 0] = [300, 0, 50, 10, 0, 0]
    log_ret[:, 0, 1] = [0, 300, 0, 0, 0, 0]
    m2 = np.array([(0, 1), (0, 1), (0, 2), (0, 2), (2, 0), (1, 1)], np.int32)
    count = np.array([1, 1, 1, 1, 0, 0], np.int32)
    tab = table_host(log_ret, np.full((E, K), 5, np.int32), np.full((E, K), TIMEOUT, np.int32), count, m2, 3, 100.0)
    opp, mine, theirs = tab.against(0)
    assert opp.tolist() == [1, 2] and mine.tolist() == [150.0, 30.0] and theirs.tolist() == [150.0, 0.0]
    assert tab.score()[0, 1] == 0.5 and tab.score()[0, 2] == 0.5 and tab.mean_length[0, 1] == 5.0 and tab.timeouts[0, 2] == 2
    assert tab.against(1)[0].size == 0
    latest, elos = pkg.elo_update(1000.0, np.array([1000.0, 1000.0]), mine, theirs)     # the existing Elo arithmetic takes the vectors
    assert latest == 1000.0 and elos.tolist() == [1000.0, 1000.0]


# ---- round_robin
def test_round_robin(pkg):
    rr = pkg.round_robin
    m2 = rr(12, [0, 1, 2])
    pairs = [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
    assert m2.dtype == np.int32 and m2.shape == (12, 2) and [tuple(r) for r in m2] == [p for p in pairs for _ in range(2)]
    assert [tuple(r) for r in rr(3, [4, 1, 2], mirror=False)] == [(1, 2), (1, 4), (2, 4)]
    sp = rr(9, [0, 1, 2], self_play=True)
    assert [tuple(r) for r in sp] == [(i, j) for i in range(3) for j in range(3)]
    assert [tuple(r) for r in rr(3, [0, 1], mirror=False, self_play=True)] == [(0, 0), (0, 1), (1, 1)]
    # the split is np.array_split's: the first E % P ranges are one env longer
    m2 = rr(8, [0, 1, 2])
    sizes = [len(idx) for idx in np.array_split(np.arange(8), 6)]
    assert [tuple(r) for r in m2] == [p for p, n in zip(pairs, sizes) for _ in range(n)] and sizes == [2, 2, 1, 1, 1, 1]
    assert [tuple(r) for r in rr(6, [0, 1, 2])] == pairs
    with pytest.raises(ValueError, match="5 envs cannot hold 6 pairs"):
        rr(5, [0, 1, 2])
    with pytest.raises(ValueError, match="twice"):
        rr(5, [0, 0])
    with pytest.raises(ValueError, match="no pairs"):
        rr(5, [3])
    assert [tuple(r) for r in rr(2, [3], self_play=True)] == [(3, 3), (3, 3)]
