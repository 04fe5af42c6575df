"""The device evaluator without a GPU: the post-step kernel's work-item function (ac_eval_post_step_host, csrc/eval_collect.hpp) driven
for consecutive steps against a numpy restatement, in this project's own words, of the bookkeeping of the runners' eval() loops
(runner/selfplay_jsbsim_runner.py:176-200; runner/jsbsim_runner.py:158-166 for the masks) plus the episode log, bit for bit; the new
header against its ctypes mirror and the exports; EvalResult and elo_update on hand-made arrays."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HID, STEPS = 128, 12
SHAPES = [(1, 1, 1), (5, 2, 1), (5, 2, 2), (3, 4, 2), (2, 8, 4), (70, 2, 1)]   # 70 envs: more than one workgroup's worth of rows
PATTERNS = ["none", "all", "one_env_every_step", "single_agent", "consecutive"]


def hashed(seed, n):
    """n float32 values in (-1, 1) from an integer hash (no generator state: the same on every machine)"""
    x = np.arange(n, dtype=np.uint64) + np.uint64((int(seed) * 0x9E3779B97F4A7C15) & (2 ** 64 - 1))
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xFF51AFD7ED558CCD)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xC4CEB9FE1A85EC53)
    x ^= x >> np.uint64(33)
    return ((x >> np.uint64(40)).astype(np.float64) / 2 ** 23 - 1.0).astype(np.float32)


def dones_for(pattern, t, E, A):
    d = np.zeros((E, A, 1), dtype=bool)
    if pattern == "all":
        d[:] = True
    elif pattern == "one_env_every_step":       # env t % E ends at step t
        d[t % E] = True
    elif pattern == "single_agent":             # one agent done while its env goes on (with A > 1); the whole env on steps 5 and 10
        d[0, A - 1] = True
        if t in (5, 10):
            d[0] = True
    elif pattern == "consecutive":              # the last env done on steps 3, 4, 5 in a row, env 0 at step 4 only
        if t in (3, 4, 5):
            d[E - 1] = True
        if t == 4:
            d[0] = True
    return d


class Loop:
    """The runners' bookkeeping after envs.step, restated: float32 cumulative rewards of both sides added once per step, the rows of
    the envs whose agents are all done appended to the episode lists and zeroed, GRU states of those envs zeroed, masks 1 - dones_env.
    The episode lists are kept as the log the evaluator keeps: env e's k-th finished episode in slot k while k < K."""

    def __init__(self, E, A, na, K, h, h_opp):
        self.E, self.A, self.na, self.K = E, A, na, K
        self.cum = np.zeros((E, A, 1), dtype=np.float32)
        self.len, self.count = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.int32)
        self.log_ret = np.zeros((E, K, A), dtype=np.float32)
        self.log_len, self.log_end = np.zeros((E, K), dtype=np.int32), np.zeros((E, K), dtype=np.int32)
        self.remaining = E
        self.h, self.h_opp = h.copy(), None if h_opp is None else h_opp.copy()
        self.masks = np.ones((E, na, 1), dtype=np.float32)
        self.opp_masks = np.ones((E, A - na, 1), dtype=np.float32)

    def step(self, t, rewards, dones):
        ended = dones[..., 0].all(axis=1)                     # [E]: every agent of the env done, the opponent's included
        alive = (~ended).astype(np.float32)
        self.masks = np.broadcast_to(alive[:, None, None], self.masks.shape).copy()
        self.opp_masks = np.broadcast_to(alive[:, None, None], self.opp_masks.shape).copy()
        self.h[ended] = 0.0
        if self.h_opp is not None:
            self.h_opp[ended] = 0.0
        self.cum += rewards                                   # float32, one add per agent and step, in step order
        self.len += 1
        for e in np.nonzero(ended)[0]:                        # the finished envs' sums go to the episode lists: here, the log
            k = self.count[e]
            if k < self.K:
                self.log_ret[e, k], self.log_len[e, k], self.log_end[e, k] = self.cum[e, :, 0], self.len[e], t
                if k == self.K - 1:
                    self.remaining -= 1
            self.count[e] += 1
        self.cum[ended] = 0
        self.len[ended] = 0


def bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("E,A,na", SHAPES)
def test_bookkeeping_matches_the_runners_eval_loops(pkg, E, A, na, K, pattern):
    lib = pkg.load_library()
    seed = 100000 * E + 1000 * A + 10 * na + K
    h = hashed(seed, E * na * HID).reshape(E, na, 1, HID)
    h_opp = hashed(seed + 1, E * (A - na) * HID).reshape(E, A - na, 1, HID) if na < A else None
    want = Loop(E, A, na, K, h, h_opp)
    got = Loop(E, A, na, K, h, h_opp)
    got.cum = got.cum.reshape(E, A)
    remaining = np.array([E], dtype=np.int32)
    ptr = lambda a: a.ctypes.data
    saw_done = False
    for t in range(STEPS):
        rewards = (hashed(seed + 7 * t + 3, E * A) * np.float32(3.7)).reshape(E, A, 1)
        dones = dones_for(pattern, t, E, A)
        if pattern == "single_agent" and A > 1 and t not in (5, 10):
            assert dones.any() and not np.all(dones[..., 0], axis=-1).any()
        # what the policy launches leave before the post-step kernel runs: new GRU states everywhere
        for side in (want, got):
            side.h = hashed(seed + 11 * t + 5, E * na * HID).reshape(E, na, 1, HID)
            if h_opp is not None:
                side.h_opp = hashed(seed + 13 * t + 6, E * (A - na) * HID).reshape(E, A - na, 1, HID)
        want.step(t, rewards, dones)
        d8 = np.ascontiguousarray(dones.astype(np.uint8))
        st = pkg.capi.AcEvalPostStep(E, A, na, HID, K, t, ptr(rewards), ptr(d8), ptr(got.h), ptr(got.masks),
                                     ptr(got.h_opp) if h_opp is not None else None, ptr(got.opp_masks) if h_opp is not None else None,
                                     ptr(got.cum), ptr(got.len), ptr(got.count), ptr(got.log_ret), ptr(got.log_len), ptr(got.log_end),
                                     ptr(remaining))
        assert lib.ac_eval_post_step_host(C.byref(st)) == 0, lib.last_error()
        assert int(remaining[0]) == want.remaining == int((want.count < K).sum()), t          # after every step
        names = ["cum", "len", "count", "log_ret", "log_len", "log_end", "h", "masks"] + (["h_opp", "opp_masks"] if h_opp is not None else [])
        for k in names:
            g, w = getattr(got, k), getattr(want, k)
            assert np.array_equal(bits(g.reshape(w.shape)), bits(w)), (k, t)
        saw_done = saw_done or np.all(dones[..., 0], axis=-1).any()
    assert saw_done == (pattern != "none")
    if pattern == "all":                                  # 12 episodes per env: K logged, the rest counted only
        assert (want.count == STEPS).all() and (want.log_len == 1).all() and (want.log_end == np.arange(K)[None, :]).all()
        assert int(remaining[0]) == 0
    if pattern == "none":
        assert (want.count == 0).all() and (want.len == STEPS).all() and not want.log_ret.any() and int(remaining[0]) == E
    if pattern == "consecutive":
        assert want.count[E - 1] == 3 and np.abs(want.cum).max() > 0


def test_episodes_beyond_the_quota_are_counted_not_logged(pkg):
    lib = pkg.load_library()
    E, A, na, K = 2, 2, 1, 2
    z = lambda *s, dt=np.float32: np.zeros(s, dtype=dt)
    h, m, ho, mo, cum = z(E * na, HID), z(E * na), z(E * (A - na), HID), z(E * (A - na)), z(E, A)
    ln, cnt, lr, ll, le = z(E, dt=np.int32), z(E, dt=np.int32), z(E, K, A), z(E, K, dt=np.int32), z(E, K, dt=np.int32)
    rem = np.array([E], dtype=np.int32)
    ptr = lambda a: a.ctypes.data
    d8 = np.array([[1, 1], [0, 1]], dtype=np.uint8)        # env 0 ends at every step, env 1 never
    for t in range(5):
        rew = np.full((E, A), t + 1, dtype=np.float32)
        st = pkg.capi.AcEvalPostStep(E, A, na, HID, K, t, ptr(rew), ptr(d8), ptr(h), ptr(m), ptr(ho), ptr(mo), ptr(cum), ptr(ln), ptr(cnt),
                                     ptr(lr), ptr(ll), ptr(le), ptr(rem))
        assert lib.ac_eval_post_step_host(C.byref(st)) == 0, lib.last_error()
        assert rem[0] == (2 if t == 0 else 1)
    assert cnt.tolist() == [5, 0] and ln.tolist() == [0, 5]
    assert lr[0].tolist() == [[1, 1], [2, 2]] and ll[0].tolist() == [1, 1] and le[0].tolist() == [0, 1]     # episodes 3 .. 5 left no trace
    assert not lr[1].any() and cum[1].tolist() == [15, 15] and cum[0].tolist() == [0, 0]
    assert m.tolist() == [0, 1] and mo.tolist() == [0, 1]


def test_host_call_refusals(pkg):
    lib = pkg.load_library()
    a = np.zeros(4096, dtype=np.float32)
    p = a.ctypes.data
    rem = np.array([2], dtype=np.int32)
    ok = [2, 2, 1, 4, 2, 0, p, p, p, p, p, p, p, p, p, p, p, p, rem.ctypes.data]
    assert lib.ac_eval_post_step_host(C.byref(pkg.capi.AcEvalPostStep(*ok))) == 0, lib.last_error()
    for idx, val, what in ((0, 0, "out of range"), (1, 9, "out of range"), (2, 3, "na"), (3, 6, "multiple of 4"), (4, 0, "episodes_per_env"),
                           (4, 65, "episodes_per_env"), (5, -1, "step must be"), (6, None, "null array"), (12, None, "null array"),
                           (18, None, "null array"), (10, None, "go together")):
        bad = list(ok)
        bad[idx] = val
        assert lib.ac_eval_post_step_host(C.byref(pkg.capi.AcEvalPostStep(*bad))) == -1
        assert what in lib.last_error(), (what, lib.last_error())
    bad = list(ok)
    bad[2] = 2                  # opponent arrays although the learner owns every agent
    assert lib.ac_eval_post_step_host(C.byref(pkg.capi.AcEvalPostStep(*bad))) == -1 and "na = A" in lib.last_error()
    assert lib.ac_eval_post_step_host(None) == -1


def test_header_and_bindings_agree(pkg, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "aircombat_eval.h"\n'
                   'int main(){printf("%zu %zu %zu %d", sizeof(ac_eval_config_t), sizeof(ac_eval_state_t), sizeof(ac_eval_post_step_t), '
                   '(int)AC_EVAL_MAX_EPISODES);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a, b, c, k = map(int, subprocess.check_output([str(exe)], text=True).split())
    capi = pkg.capi
    assert a == C.sizeof(capi.AcEvalConfig) == 20 and b == C.sizeof(capi.AcEvalState) and c == C.sizeof(capi.AcEvalPostStep)
    assert k == capi.AC_EVAL_MAX_EPISODES == 64
    hdr = open(os.path.join(ROOT, "include", "aircombat_eval.h")).read()
    declared = set(re.findall(r"\b(ac_eval_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"ac_eval_create", "ac_eval_destroy", "ac_eval_begin", "ac_eval_run", "ac_eval_state", "ac_eval_post_step_host"}
    lib = pkg.load_library()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib.path], text=True)
    for sym in declared:
        assert sym in capi.SIGNATURES and hasattr(lib, sym) and re.search(rf"\bT {sym}\b", exported), sym
    assert set(re.findall(r"\bT (ac_eval_[a-z0-9_]+)\b", exported)) == declared
    assert (capi.AC_EVAL_NO_OPPONENT, capi.AC_EVAL_OPPONENT_POLICY, capi.AC_EVAL_OPPONENT_POOL) == (0, 1, 2)


def test_exports_and_null_handles(pkg):
    for name in ("DeviceEvaluator", "EvalResult", "elo_update"):
        assert getattr(pkg, name).__name__ == name and name in pkg.__all__
    lib = pkg.load_library()
    out = C.c_void_p()
    assert lib.ac_eval_create(None, None, None, None, C.byref(out)) == -1 and "null argument" in lib.last_error()
    assert lib.ac_eval_run(None, None, 1, 0, 0, 0, 0) == -1 and "null handle" in lib.last_error()
    assert lib.ac_eval_begin(None, None) == -1 and "null handle" in lib.last_error()
    assert lib.ac_eval_state(None, None) == -1
    assert lib.ac_eval_destroy(None) == 0


def elo_by_hand(learner_elo, opponent_elos, learner_avg, opponent_avg, k=32.0, threshold=100.0):
    """The self-play runner's Elo rule worked out one opponent at a time in Python floats: the opponent's expected score from the
    logistic curve on the rating gap over 400, its actual score from how far its average episode reward lies above the learner's
    (a win strictly above +threshold, a tie strictly inside, otherwise nothing), the gain k * (actual - expected) credited to the
    opponent and debited from a copy of the learner's rating per opponent; the learner's new rating is the mean of the copies.
    Returns (new learner rating, new opponent ratings, the actual scores)."""
    new_ratings, learner_copies, scores = [], [], []
    for rating, mine, theirs in zip(opponent_elos, learner_avg, opponent_avg):
        gap = float(theirs) - float(mine)
        if gap > threshold:
            score = 1.0
        elif -threshold < gap < threshold:
            score = 0.5
        else:
            score = 0.0
        expected = 1.0 / (1.0 + math.pow(10.0, (rating - learner_elo) / 400.0))
        gain = k * (score - expected)
        new_ratings.append(rating + gain)
        learner_copies.append(learner_elo - gain)
        scores.append(score)
    return math.fsum(learner_copies) / len(learner_copies), new_ratings, scores


# Ratings are about 1e3 and each is a handful of float64 operations (eps = 2.2e-16) plus one pow, whose vectorised and scalar forms may
# differ by an ulp: the two computations agree to a few 1e-13. One step of the actual score moves a rating by 16, so 1e-10 separates them.
ELO_TOL = 1e-10


def test_elo_update_matches_the_reference_lines(pkg):
    gaps = np.array([250.0, 100.5, 100.0, 99.5, 0.0, -99.5, -100.0, -100.5, -250.0])     # both sides of +-100 and exactly at them
    learner = np.array([30.0, -12.5, 7.0, 0.25, 100.0, -40.0, 3.0, 55.5, 1000.0])
    opponent = learner + gaps
    assert np.array_equal(opponent - learner, gaps)
    ratings = [1000.0 + 37.5 * i - 3.0 * i * i for i in range(len(gaps))]
    latest = 1043.25
    want_latest, want_ratings, scores = elo_by_hand(latest, ratings, learner, opponent)
    assert scores == [1.0, 1.0, 0.0, 0.5, 0.5, 0.5, 0.0, 0.0, 0.0]
    got_latest, got_ratings = pkg.elo_update(latest, ratings, learner, opponent)
    assert got_ratings.dtype == np.float64 and isinstance(got_latest, float)
    assert np.abs(got_ratings - np.array(want_ratings)).max() < ELO_TOL and abs(got_latest - want_latest) < ELO_TOL
    # the sign convention: a winning opponent (score 1) gains, and the learner loses what the opponents gain on average
    assert got_ratings[0] > ratings[0] and got_ratings[-1] < ratings[-1]
    assert abs((got_latest - latest) + (got_ratings - np.array(ratings)).mean()) < ELO_TOL
    # other k and threshold
    want2 = elo_by_hand(1000.0, [1000.0, 1200.0], [0.0, 0.0], [5.0, 20.0], k=16.0, threshold=10.0)
    l2, e2 = pkg.elo_update(1000.0, [1000.0, 1200.0], [0.0, 0.0], [5.0, 20.0], k=16.0, threshold=10.0)
    assert want2[2] == [0.5, 1.0] and np.abs(e2 - np.array(want2[1])).max() < ELO_TOL and abs(l2 - want2[0]) < ELO_TOL
    # refused before anything is computed: vectors of different lengths, and an average that is not finite (a member with no logged
    # episode comes out of per_opponent() as NaN; it must not be scored as a loss)
    with pytest.raises(ValueError, match="one entry per opponent"):
        pkg.elo_update(1000.0, [1000.0, 1200.0], [0.0], [5.0, 20.0, 1.0])
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="not finite"):
            pkg.elo_update(1000.0, [1000.0, 1200.0], [0.0, bad], [5.0, 20.0])
        with pytest.raises(ValueError, match="not finite"):
            pkg.elo_update(1000.0, [1000.0, 1200.0], [0.0, 1.0], [bad, 20.0])



def hand_made(pkg):
    """E = 4, K = 2, A = 2, na = 1. Episodes (env, end step): (0, 3), (0, 9), (1, 3), (1, 5) and a third at some later step that was
    not logged, (2, 7), none for env 3."""
    ret = np.zeros((4, 2, 2), dtype=np.float32)
    ret[0, 0], ret[0, 1], ret[1, 0], ret[1, 1], ret[2, 0] = [1, -1], [2, -2], [3, -3], [4, -4], [5, -5]
    ret[2, 1] = [99, 99]                                    # a slot that holds no episode: never shown
    lengths = np.array([[4, 6], [4, 2], [8, 0], [0, 0]], dtype=np.int32)
    ends = np.array([[3, 9], [3, 5], [7, 0], [0, 0]], dtype=np.int32)
    counts = np.array([2, 3, 1, 0], dtype=np.int32)
    return pkg.EvalResult(ret, lengths, ends, counts, np.array([0, 0, 1, 1], dtype=np.int32), 12, 1)


def test_episodes_come_in_the_reference_order(pkg):
    r = hand_made(pkg)
    ep = r.episodes()
    assert ep.envs.tolist() == [0, 1, 1, 2, 0] and ep.end_steps.tolist() == [3, 3, 5, 7, 9]       # by end step, then by env
    assert ep.returns[:, 0].tolist() == [1, 3, 4, 5, 2] and ep.lengths.tolist() == [4, 4, 2, 8, 6]
    assert ep.returns.shape == (5, 2) and ep.returns.dtype == np.float32
    assert r.logged.tolist() == [[True, True], [True, True], [True, False], [False, False]]
    first = r.episodes(3)                                     # env 1's log fills at step 5, the third episode's own end: nothing missed
    assert first.envs.tolist() == [0, 1, 1] and first.end_steps.tolist() == [3, 3, 5]
    assert r.episodes(0).returns.shape == (0, 2)
    for n in (4, 5):                                          # env 1 was full from step 5 on and finished a third episode: when is not known
        with pytest.raises(ValueError, match="env 1 filled its 2 log slots at step 5"):
            r.episodes(n)
    with pytest.raises(ValueError, match="6 asked for, 5 logged"):
        r.episodes(6)
    # an env that is full but finished nothing further hides nothing
    r.counts[1] = 2
    assert r.episodes(5).envs.tolist() == [0, 1, 1, 2, 0]


def test_per_opponent_on_a_hand_made_log(pkg):
    E, K, A, na = 6, 3, 4, 2
    ret = (np.arange(E * K * A, dtype=np.float32).reshape(E, K, A) * np.float32(0.37) - np.float32(11.3)).astype(np.float32)
    counts = np.array([3, 1, 5, 0, 2, 1], dtype=np.int32)                 # env 2: two episodes beyond the quota
    members = np.array([2, 0, 2, 0, 5, 5], dtype=np.int32)                # member 2: 3 + 3 episodes, member 0: 1 + 0, member 5: 2 + 1
    r = pkg.EvalResult(ret, np.ones((E, K), np.int32), np.zeros((E, K), np.int32), counts, members, 9, na)
    got = r.per_opponent()
    assert got["members"].tolist() == [0, 2, 5] and got["episodes"].tolist() == [1, 6, 3]
    eps = {0: [ret[1, 0]], 2: [ret[0, 0], ret[0, 1], ret[0, 2], ret[2, 0], ret[2, 1], ret[2, 2]], 5: [ret[4, 0], ret[4, 1], ret[5, 0]]}
    for i, m in enumerate([0, 2, 5]):
        rows = np.stack(eps[m])
        ours, theirs = rows[:, :na].mean(axis=1), rows[:, na:].mean(axis=1)          # per episode: the float32 mean over the side's agents
        assert ours.dtype == np.float32
        assert got["learner"][i] == ours.astype(np.float64).mean()
        assert got["opponent"][i] == theirs.astype(np.float64).mean()
    assert got["learner"].dtype == np.float64
    # a member with no logged episode: counted as 0, averages NaN; without an opponent side the opponent's average is NaN
    r2 = pkg.EvalResult(ret, np.ones((E, K), np.int32), np.zeros((E, K), np.int32), np.array([1, 0, 0, 0, 0, 0], np.int32), members, 9, A)
    g2 = r2.per_opponent()
    assert g2["episodes"].tolist() == [0, 1, 0] and np.isnan(g2["learner"][[0, 2]]).all() and np.isnan(g2["opponent"]).all()
    assert g2["learner"][1] == ret[0, 0].mean(dtype=np.float32).astype(np.float64)
