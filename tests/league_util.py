"""Shared by the league's tests (test_league_host.py, test_gpu_league.py): the payoff table restated in numpy scalars in the contract's
two-level summation order (include/aircombat_league.h), and a synthetic log whose reward differences sit at and around the margin."""
import numpy as np

TIMEOUT = 7   # AC_DONE_TIMEOUT


def table_loop(log_ret, log_len, log_code, count, m2, Cn, margin):
    """The contract's two-level order in numpy scalars: per env over its slots ascending from 0.0, per cell over its envs ascending."""
    E, K, A = log_ret.shape
    half = A // 2
    margin = np.float32(margin)
    part = []
    for e in range(E):
        c = dict(episodes=0, wins_a=0, wins_b=0, draws=0, timeouts=0, steps=0, sum_a=np.float64(0.0), sum_b=np.float64(0.0))
        for k in range(min(int(count[e]), K)):
            side = []
            for a0 in (0, half):
                s = np.float32(log_ret[e, k, a0])
                for a in range(a0 + 1, a0 + half):
                    s = np.float32(s + log_ret[e, k, a])
                side.append(np.float32(s / np.float32(half)))
            ra, rb = side
            d = np.float32(ra - rb)
            c["episodes"] += 1
            c["wins_a"] += int(d > margin)
            c["wins_b"] += int(d < -margin)
            c["draws"] += int(not (d > margin) and not (d < -margin))
            c["timeouts"] += int(log_code[e, k] == TIMEOUT)
            c["steps"] += int(log_len[e, k])
            c["sum_a"] = c["sum_a"] + np.float64(ra)
            c["sum_b"] = c["sum_b"] + np.float64(rb)
        part.append(c)
    out = {k: np.zeros((Cn, Cn), dtype=np.float64 if k.startswith("sum") else np.int64) for k in part[0]}
    for i in range(Cn):
        for j in range(Cn):
            for e in range(E):
                if (m2[e, 0], m2[e, 1]) == (i, j):
                    for k in out:
                        out[k][i, j] = out[k][i, j] + part[e][k]
    return out


def assert_table(tab, want):
    for k, w in want.items():
        g = getattr(tab, k)
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (k, g, w)


def threshold_log(E, K, A, margin):
    """A synthetic log: env e's slot k holds side rewards whose float32 difference sits at, just inside and just beyond +margin and
    -margin in turn, the rest hashed values; counts run from 0 to beyond K."""
    rng = np.random.default_rng(E * 31 + A)
    log_ret = (rng.standard_normal((E, K, A)) * 120).astype(np.float32)
    m = np.float32(margin)
    diffs = [m, -m, np.nextafter(m, np.float32(np.inf)), np.nextafter(-m, np.float32(-np.inf)), np.nextafter(m, np.float32(0)),
             np.nextafter(-m, np.float32(0)), np.float32(0)]
    for e in range(min(E, len(diffs))):
        log_ret[e, 0, :A // 2] = diffs[e]      # side a's mean is the difference itself (a sum of equal small powers-of-two multiples is exact for A/2 in 1, 2, 4)
        log_ret[e, 0, A // 2:] = 0.0
    log_len = rng.integers(1, 40, size=(E, K)).astype(np.int32)
    log_code = rng.integers(1, 9, size=(E, K)).astype(np.int32)
    count = (np.arange(E) % (K + 2)).astype(np.int32)          # 0 .. K + 1: empty envs, partly filled, full, and count > K
    count[:len(diffs)] = np.maximum(count[:len(diffs)], 1)
    return log_ret, log_len, log_code, count
