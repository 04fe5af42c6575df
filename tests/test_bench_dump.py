"""bench.py --dump-outputs: what the last timed step handed its caller, written as .npy files (float32 / float64, at most 64 MB in all),
the same from run to run with the same arguments."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Infos:
    def __init__(self, codes):
        self._codes = codes


def test_info_words_decode_to_columns():
    b = _bench()
    # current_step 17, done code 8, heading_turn_counts 3, env reset; and a plain running env
    words = np.array([17 | 8 << 16 | 3 << 24 | 1 << 31, 5], dtype=np.uint32).view(np.int32)
    cols = b.info_columns(np, words)
    assert cols.dtype == np.float64 and cols.tolist() == [[17, 8, 3, 1], [5, 0, 0, 0]]
    rows = np.array([[17, 8, 3, 1], [5, 0, 0, 0]], dtype=np.int32)
    assert b.info_columns(np, rows).tolist() == cols.tolist()


def test_step_outputs_are_float_copies():
    b = _bench()
    E, A, D = 3, 4, 5
    obs = np.arange(E * A * D, dtype=np.float32).reshape(E, A, D)
    rew = np.ones((E, A, 1), np.float32)
    done = np.zeros((E, A, 1), bool)
    share = np.broadcast_to(obs.reshape(E, 1, A * D), (E, A, A * D))
    infos = _Infos(np.zeros(E, np.int32))
    two = b.step_outputs(np, (obs, rew, done, infos))
    assert sorted(two) == ["dones", "infos", "obs", "rewards"]
    many = b.step_outputs(np, (obs, share, rew, done, infos))
    assert sorted(many) == ["dones", "infos", "obs", "rewards", "share_obs"] and many["share_obs"].shape == (E, A, A * D)
    for a in many.values():
        assert a.dtype in (np.float32, np.float64) and a.flags.owndata
    assert np.shares_memory(many["obs"], obs) is False


def test_dump_is_complete_under_the_cap_and_a_fixed_sample_over_it(tmp_path, monkeypatch):
    b = _bench()
    E = 1000
    arrays = {"obs": np.random.default_rng(1).random((E, 2, 15)).astype(np.float32), "infos": np.arange(E * 4, dtype=np.float64).reshape(E, 4)}
    b.dump_outputs(np, arrays, str(tmp_path / "all"))
    assert sorted(os.listdir(tmp_path / "all")) == ["infos.npy", "obs.npy"]
    assert (np.load(tmp_path / "all" / "obs.npy") == arrays["obs"]).all()
    monkeypatch.setattr(b, "DUMP_BYTES_MAX", 64 * 10 ** 3)
    for run in ("s1", "s2"):
        b.dump_outputs(np, arrays, str(tmp_path / run))
    files = sorted(os.listdir(tmp_path / "s1"))
    assert files == ["infos.npy", "obs.npy", "sample_env_index.npy"]
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in files) <= 64 * 10 ** 3       # .npy headers included
    idx = np.load(tmp_path / "s1" / "sample_env_index.npy").astype(np.int64)
    assert len(idx) < E and (np.diff(idx) > 0).all()
    assert (np.load(tmp_path / "s1" / "obs.npy") == arrays["obs"][idx]).all()
    assert (np.load(tmp_path / "s1" / "infos.npy") == arrays["infos"][idx]).all()
    for f in files:
        assert (np.load(tmp_path / "s1" / f) == np.load(tmp_path / "s2" / f)).all()


def test_dump_refuses_the_stub_env(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--stub-env", "--dump-outputs", str(tmp_path / "d")],
                         capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert out.returncode != 0 and "--dump-outputs" in out.stderr
    assert not os.path.exists(tmp_path / "d")


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step_identically_from_run_to_run(tmp_path):
    """Two runs with the same arguments dump the same arrays, bit for bit, with the shapes VecEnv.step returns."""
    runs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3", "--envs", "64",
               "--no-cpu-baseline", "--no-configs", "--no-saturating", "--no-steady-state", "--dump-outputs", str(d)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert out.returncode == 0, out.stderr[-2000:]
        r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
        assert r["steps"] == 7 and r["warmup"] == 3
        runs.append({f[:-4]: np.load(d / f) for f in os.listdir(d)})
    a, b = runs
    assert sorted(a) == ["dones", "infos", "obs", "rewards"] and sorted(b) == sorted(a)
    assert a["obs"].shape == (64, 2, 15) and a["obs"].dtype == np.float32
    assert a["rewards"].shape == (64, 2, 1) and a["dones"].shape == (64, 2, 1) and a["infos"].shape == (64, 4)
    assert np.isfinite(a["obs"]).all() and np.isfinite(a["rewards"]).all()
    for k in a:
        assert a[k].dtype in (np.float32, np.float64)
        assert np.array_equal(a[k], b[k]), k
