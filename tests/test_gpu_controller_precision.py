"""The reference-precision form of the low-level controller (AC_CTL_FP32: three bf16 pieces per value, six terms per product) on the device:
its products at least as exact as the reference's own fp32 arithmetic (an all-fp32 numpy restatement of BaselineActor, below), measured
against the float64 oracle (oracle.actor_forward) on the golden sequences and on batches of every shape; the env path under
AIRCOMBAT_CTL_PRECISION=fp32; the weight check of the form."""
import os

import numpy as np
import pytest

from test_gpu_parity import _lowlevel_controller_parity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "baseline_actor.npz")
FLIP_GAP = 1e-4
HEADS = (0, 41, 82, 123, 153)


def _weights():
    return np.fromfile(os.path.join(ROOT, "aircombat-selfplay_amd", "data", "baseline_actor.f32"), dtype=np.float32)


class Fp32Actor:
    """BaselineActor (baseline_actor.py) in float32 throughout, like torch on the CPU: the reference's arithmetic."""

    def __init__(self, w):
        o = 0

        def take(*shape):
            nonlocal o
            n = int(np.prod(shape))
            a = w[o:o + n].reshape(shape).astype(np.float32)
            o += n
            return a
        self.w1, self.b1, self.g1, self.be1 = take(128, 12), take(128), take(128), take(128)
        self.w2, self.b2, self.g2, self.be2 = take(128, 128), take(128), take(128), take(128)
        self.wih, self.whh, self.bih, self.bhh = take(384, 128), take(384, 128), take(384), take(384)
        self.g3, self.be3 = take(128), take(128)
        self.wa, self.ba = take(153, 128), take(153)
        assert o == w.size

    @staticmethod
    def _ln(x, g, b):
        m = x.mean(axis=-1, keepdims=True, dtype=np.float32)
        v = ((x - m) ** 2).mean(axis=-1, keepdims=True, dtype=np.float32)
        return ((x - m) / np.sqrt(v + np.float32(1e-5))) * g + b

    def __call__(self, x, h):
        x = x.astype(np.float32)
        h = h.astype(np.float32)
        a = self._ln(np.maximum(x @ self.w1.T + self.b1, 0), self.g1, self.be1)
        a = self._ln(np.maximum(a @ self.w2.T + self.b2, 0), self.g2, self.be2)
        gi = a @ self.wih.T + self.bih
        gh = h @ self.whh.T + self.bhh
        sig = lambda v: np.float32(1) / (np.float32(1) + np.exp(-v))
        r = sig(gi[:, :128] + gh[:, :128])
        z = sig(gi[:, 128:256] + gh[:, 128:256])
        n = np.tanh(gi[:, 256:] + r * gh[:, 256:])
        hn = (np.float32(1) - z) * n + z * h
        return hn, self._ln(hn, self.g3, self.be3) @ self.wa.T + self.ba


def _oracle_rows(oracle, x, h):
    oracle.actor_load()
    acts, hs, lgs = [], [], []
    for xi, hi in zip(x, h):
        a, hn, lg = oracle.actor_forward(xi, hi)
        acts.append(a); hs.append(hn); lgs.append(lg)
    return np.array(acts), np.array(hs), np.array(lgs)


_GOLDEN_NP32 = []


def _np32_golden_errors(oracle):
    """max |d state|, max |d logit| of the numpy fp32 restatement against the float64 oracle on the golden sequences, free-running from a
    zero state: the bound the fp32 form is held to (the reference's own arithmetic on the reference's own inputs)"""
    if not _GOLDEN_NP32:
        X = np.load(GOLDEN)["x"].astype(np.float32)
        ref32 = Fp32Actor(_weights())
        h32, h64, eh, el = np.zeros((X.shape[0], 128), np.float32), np.zeros((X.shape[0], 128)), 0.0, 0.0
        for t in range(X.shape[1]):
            _, h64, rl = _oracle_rows(oracle, X[:, t].astype(np.float64), h64)
            h32, l32 = ref32(X[:, t], h32)
            eh, el = max(eh, float(np.abs(h32 - h64).max())), max(el, float(np.abs(l32 - rl).max()))
        _GOLDEN_NP32.extend([eh, el])
    return tuple(_GOLDEN_NP32)


def _check_argmax(act, ref_lg):
    """device argmax == oracle argmax, except where the oracle's own top-two gap of that head is below FLIP_GAP"""
    flips = 0
    for hd in range(4):
        seg = ref_lg[:, HEADS[hd]:HEADS[hd + 1]]
        srt = np.sort(seg, axis=1)
        gap = srt[:, -1] - srt[:, -2]
        bad = act[:, hd] != seg.argmax(axis=1)
        assert (gap[bad] < FLIP_GAP).all(), (hd, np.flatnonzero(bad), gap[bad])
        flips += int(bad.sum())
    return flips


def test_golden_sequences_free_running(pkg, oracle):
    g = np.load(GOLDEN)
    X = g["x"].astype(np.float32)      # [16 sequences][24 steps][12]
    S, T = X.shape[:2]
    ref32 = Fp32Actor(_weights())
    h = {"fast": np.zeros((S, 128), np.float32), "fp32": np.zeros((S, 128), np.float32), "np32": np.zeros((S, 128), np.float32)}
    h64 = np.zeros((S, 128))
    err = {k: [0.0, 0.0] for k in h}
    flips = {"fast": 0, "fp32": 0}
    for t in range(T):
        ra, h64, rl = _oracle_rows(oracle, X[:, t].astype(np.float64), h64)
        for prec in ("fast", "fp32"):
            act, h[prec], lg = pkg.controller_forward(X[:, t], h[prec], precision=prec)
            err[prec][0] = max(err[prec][0], float(np.abs(h[prec] - h64).max()))
            err[prec][1] = max(err[prec][1], float(np.abs(lg - rl).max()))
            flips[prec] += _check_argmax(act, rl)
        h["np32"], lg32 = ref32(X[:, t], h["np32"])
        err["np32"][0] = max(err["np32"][0], float(np.abs(h["np32"] - h64).max()))
        err["np32"][1] = max(err["np32"][1], float(np.abs(lg32 - rl).max()))
    print(f"golden {S}x{T}, free-running, max |d state| / max |d logit| against float64: fp32 form {err['fp32'][0]:.2e} / "
          f"{err['fp32'][1]:.2e}, numpy fp32 (the reference's arithmetic) {err['np32'][0]:.2e} / {err['np32'][1]:.2e}, "
          f"fast form {err['fast'][0]:.2e} / {err['fast'][1]:.2e}; argmax flips on near-ties: fp32 {flips['fp32']}, fast {flips['fast']}")
    assert err["fp32"][0] <= err["np32"][0] and err["fp32"][1] <= err["np32"][1], err
    assert tuple(err["np32"]) == _np32_golden_errors(oracle)
    # the test tells the forms apart: the fast form's products are measurably less exact
    assert err["fast"][0] > err["fp32"][0] and err["fast"][1] > err["fp32"][1], err


@pytest.mark.parametrize("rows", ["32", "64"])
def test_batch_shapes(pkg, oracle, monkeypatch, rows):
    monkeypatch.setenv("AIRCOMBAT_CTL_ROWS", rows)
    g = np.load(GOLDEN)
    pool = g["x"].reshape(-1, 12).astype(np.float32)
    bound_h, bound_l = _np32_golden_errors(oracle)
    rng = np.random.default_rng(int(rows))
    for n in (1, 31, 1000, 8192, 32768 + 17):
        x = pool[rng.integers(0, len(pool), size=n)]
        h = rng.uniform(-1.0, 1.0, size=(n, 128)).astype(np.float32)
        tile = int(rows)
        last = np.arange((n - 1) // tile * tile, n)                  # the last (partial) workgroup, whole
        pick = np.unique(np.concatenate([last, rng.choice(n, size=min(n, 512 - len(last)), replace=False)]))
        ra, rh, rl = _oracle_rows(oracle, x[pick].astype(np.float64), h[pick].astype(np.float64))
        errs = {}
        for prec in ("fp32", "fast"):
            act, hn, lg = pkg.controller_forward(x, h, precision=prec)
            assert act.shape == (n, 4) and hn.shape == (n, 128) and lg.shape == (n, 153)
            eh, el = float(np.abs(hn[pick] - rh).max()), float(np.abs(lg[pick] - rl).max())
            errs[prec] = (eh, el)
            _check_argmax(act[pick], rl)
            if prec == "fp32":
                assert eh <= bound_h and el <= bound_l, (n, rows, eh, bound_h, el, bound_l)
            else:
                assert eh < 5e-5 and el < 2e-4, (n, rows, eh, el)
        print(f"rows {rows} n {n}: {len(pick)} rows compared, max |d state| / |d logit|: fp32 form {errs['fp32'][0]:.2e} / {errs['fp32'][1]:.2e}"
              f" (bound {bound_h:.2e} / {bound_l:.2e}), fast form {errs['fast'][0]:.2e} / {errs['fast'][1]:.2e}")


@pytest.mark.parametrize("task,baseline,per_side", [("hierarchical_singlecombat", 0, None), ("hierarchical_singlecombat", 1, None),
                                                    ("hierarchical_singlecombat", 2, None), ("scenario1", 0, None),
                                                    ("scenario_nvn", 0, 2)])
def test_env_path_under_fp32_pin(pkg, oracle, monkeypatch, task, baseline, per_side):
    monkeypatch.setenv("AIRCOMBAT_CTL_PRECISION", "fp32")
    probe = pkg.HipVecEnv(pkg.default_config("hierarchical_singlecombat"), 2)
    assert probe.controller_precision == "fp32"     # the pin reaches the handles the helper makes
    probe.close()
    if per_side:
        _lowlevel_controller_parity(pkg, oracle, task, baseline, E=5, per_side=per_side, steps=90)
    else:
        _lowlevel_controller_parity(pkg, oracle, task, baseline)


def test_handle_reports_its_form(pkg, monkeypatch):
    monkeypatch.delenv("AIRCOMBAT_CTL_PRECISION", raising=False)
    cfg = pkg.default_config("hierarchical_singlecombat")
    a = pkg.HipVecEnv(cfg, 4, controller_precision="fp32")
    b = pkg.HipVecEnv(cfg, 4)
    c = pkg.make_env(num_envs=2, task="hierarchical_singlecombat", controller_precision="fp32")
    try:
        assert (a.controller_precision, b.controller_precision, c.controller_precision) == ("fp32", "fast", "fp32")
        a.reset(); b.reset()
        act = np.zeros((4, 2, 3), dtype=np.float32)
        a.step(act); b.step(act)
    finally:
        a.close(); b.close(); c.close()
    with pytest.raises(RuntimeError, match="hierarchical"):
        pkg.HipVecEnv(pkg.default_config("singlecombat"), 2, controller_precision="fp32")


def test_fp32_form_refuses_non_finite_weights(pkg):
    from aircombat_selfplay_amd import capi
    env = pkg.HipVecEnv(pkg.default_config("hierarchical_singlecombat"), 2, controller_precision="fp32")
    try:
        w = _weights().copy()
        w[4000] = np.nan
        with pytest.raises(RuntimeError, match="non-finite"):
            env.lib.check(env.lib.ac_load_controller(env._h, w.ctypes.data, int(w.size)), "ac_load_controller")
        with pytest.raises(RuntimeError, match="non-finite"):
            pkg.controller_forward(np.zeros(12), np.zeros(128), precision="fp32", weights=w)
    finally:
        env.close()
    assert capi.AC_CTL_FP32 == 1
