"""The native VecEnv.step (csrc/native_step.cpp) without a GPU: the extension runs against tests/host/native_step_stub.c, a stand-in for
ac_step_host_actions_begin / _wait compiled here, over result sets made of ordinary numpy arrays. Checked: which set it picks for every
hold pattern of a four-set ring, what it passes to the library, that the result exists before the wait and the GIL is free during it,
and that every input or ring state it does not take is answered with None and nothing changed. The set-picking rule on its own
(csrc/native_step_pick.hpp) also runs as a program of its own under the address and undefined-behaviour sanitizers."""
import ctypes as C
import itertools
import os
import shutil
import subprocess
import threading
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, A, ACT, OBS = 6, 2, 4, 5
N_FLOATS = E * A * ACT


class Stub(C.Structure):
    _fields_ = [("obs", C.c_void_p * 8), ("begin_calls", C.c_int32), ("wait_calls", C.c_int32), ("last_set", C.c_int32), ("last_actions", C.c_void_p),
                ("last_n", C.c_size_t), ("first", C.c_double), ("last", C.c_double), ("sum", C.c_double), ("begin_rc", C.c_int32), ("wait_rc", C.c_int32),
                ("wait_ms", C.c_int32), ("wait_t0", C.c_double), ("wait_t1", C.c_double), ("last_handle", C.c_void_p)]


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    if g.build_native() is None:
        pytest.skip("no Python.h or host compiler here: the native step is not built (build() says so)")
    import aircombat_selfplay_amd as pkg
    assert pkg.vec_env._native_step is not None
    return pkg.vec_env._native_step


@pytest.fixture(scope="module")
def stub_dll(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "no host C compiler"
    so = tmp_path_factory.mktemp("native_step_stub") / "libnative_step_stub.so"
    subprocess.check_call([cc, "-O1", "-g", "-fPIC", "-shared", os.path.join(ROOT, "tests", "host", "native_step_stub.c"), "-o", str(so)])
    dll = C.CDLL(str(so))
    dll.stub_state.restype = C.POINTER(Stub)
    return dll


class FakeEnv:
    """What the native step touches of a HipVecEnv: `_cur`."""

    def __init__(self):
        self._cur = 0


class Infos:
    """Stands for LazyInfos; notes how many waits the stub had seen when it was built."""
    stub = None

    def __init__(self, codes):
        self._codes = codes
        self.waits_seen = Infos.stub.wait_calls
        self.begins_seen = Infos.stub.begin_calls


HANDLE = 0x5EED0


class Rig:
    def __init__(self, native, dll, n_sets, copy=True, share=False):
        self.stub = dll.stub_state().contents
        C.memset(C.byref(self.stub), 0, C.sizeof(Stub))
        Infos.stub = self.stub
        self.errors = []
        self.env = FakeEnv()
        self.outs, self.results = [], []

        def check(rc, what):
            self.errors.append((rc, what))
            if rc != 0:
                raise RuntimeError(f"{what} failed: stub")

        self.stepper = native.Stepper(C.cast(dll.stub_begin, C.c_void_p).value, C.cast(dll.stub_wait, C.c_void_p).value, HANDLE, N_FLOATS, copy, share,
                                      Infos, check)
        for k in range(n_sets):
            obs = np.zeros((E, A, OBS), dtype=np.float32)
            out = (obs, np.zeros((E, A, 1), dtype=np.float32), np.zeros((E, A, 1), dtype=bool), np.zeros(E, dtype=np.int32))
            if share:
                out = out + (np.broadcast_to(obs.reshape(E, 1, A * OBS), (E, A, A * OBS)),)
            self.stub.obs[k] = obs.ctypes.data
            res = ((out[0], out[4], out[1], out[2], Infos(out[3])) if share else (out[0], out[1], out[2], Infos(out[3])))
            self.outs.append(out)
            self.results.append(res)
            del obs
            self.stepper.add_set(out, res)
            del out, res

    def step(self, a):
        return self.stepper.step(self.env, a)


def batch(seed=0):
    return np.random.default_rng(seed).integers(0, 30, size=(E, A, ACT)).astype(np.float32)


def expected_pick(cur, held):
    """HipVecEnv._next_set's ring rule, written out: the first set after `cur` in ring order that nobody holds, `cur` itself last."""
    n = len(held)
    for i in range(1, n + 1):
        k = (cur + i) % n
        if not held[k]:
            return k
    return None


@pytest.mark.parametrize("which", range(4))   # which of the set's four arrays the caller keeps
def test_set_choice_for_every_hold_pattern_of_a_four_set_ring(native, stub_dll, which):
    rig = Rig(native, stub_dll, 4)
    a = batch()
    for pattern in itertools.product((False, True), repeat=4):
        for cur in range(4):
            rig.env._cur = cur
            holds = [rig.outs[k][which][...] if h else None for k, h in enumerate(pattern)]    # a view counts like the array itself
            assert [rig.stepper.held(k) for k in range(4)] == list(pattern)
            before = rig.stub.begin_calls
            res = rig.step(a)
            want = expected_pick(cur, pattern)
            if want is None:                       # every set held: the Python path stages and copies
                assert res is None and rig.stub.begin_calls == before and rig.env._cur == cur
            else:
                assert rig.stub.last_set == want and rig.env._cur == want and rig.stub.begin_calls == before + 1
                assert all(x is y for x, y in zip(res[:3], rig.outs[want][:3])) and res[3]._codes is rig.outs[want][3]
                assert res[0][0, 0, 0] == rig.stub.begin_calls      # the stub "stepped" into that set's buffer
            del holds, res
    assert rig.errors == []


def test_a_result_the_caller_keeps_holds_its_set_and_a_dropped_one_frees_it(native, stub_dll):
    rig = Rig(native, stub_dll, 4)
    a = batch()
    r0 = rig.step(a)
    r1 = rig.step(a)
    infos_only = rig.step(a)[3]                    # the LazyInfos alone keeps the info words, and with them the set
    picked = [rig.stub.last_set]
    for _ in range(4):
        r = rig.step(a)
        picked.append(rig.stub.last_set)
        del r
    assert (r0[0] is rig.outs[1][0]) and (r1[0] is rig.outs[2][0]) and picked == [3, 0, 0, 0, 0]
    del r0, infos_only
    got = []
    for _ in range(4):
        r = rig.step(a)
        got.append(rig.stub.last_set)
        del r
    assert got == [1, 3, 0, 1]
    del r1


def test_argument_values_and_the_result_exists_before_the_wait(native, stub_dll):
    rig = Rig(native, stub_dll, 2)
    a = batch(3)
    ro = batch(4)
    ro.flags.writeable = False
    flat = batch(5).reshape(-1)                    # any shape of the right size, as the Python path takes it
    for k, arr in enumerate((a, ro, flat)):
        res = rig.step(arr)
        s = rig.stub
        assert s.last_handle == HANDLE and s.last_n == N_FLOATS and s.last_actions == arr.ctypes.data and s.last_set == (k + 1) % 2
        assert (s.first, s.last, s.sum) == (float(arr.flat[0]), float(arr.flat[-1]), float(arr.astype(np.float64).sum()))
        assert (s.begin_calls, s.wait_calls) == (k + 1, k + 1)
        assert (res[3].begins_seen, res[3].waits_seen) == (k + 1, k)     # built after the doorbell, before the wait
        del res
    assert rig.errors == []


def test_copy_false_alternates_two_sets_and_returns_their_prebuilt_results(native, stub_dll):
    rig = Rig(native, stub_dll, 2, copy=False)
    a = batch()
    kept = [rig.step(a) for _ in range(5)]         # holding everything changes nothing in this mode
    assert [k is rig.results[i % 2] for i, k in zip((1, 0, 1, 0, 1), kept)] == [True] * 5
    assert rig.env._cur == 1 and rig.stub.begin_calls == 5


def test_share_family_result_order(native, stub_dll):
    rig = Rig(native, stub_dll, 2, share=True)
    obs, share_obs, rew, done, infos = rig.step(batch())
    o = rig.outs[1]
    assert obs is o[0] and share_obs is o[4] and rew is o[1] and done is o[2] and infos._codes is o[3]
    assert not share_obs.flags.owndata and np.shares_memory(share_obs, obs)     # still the broadcast view
    del obs, rew, done, infos
    rig.step(batch())
    assert rig.stub.last_set == 0                  # share_obs alone holds set 1
    rig.step(batch())
    assert rig.stub.last_set == 0


@pytest.mark.parametrize("name", ["nested lists", "float64", "int32", "strided slice", "transposed", "too few", "too many", "not a buffer", "big-endian"])
def test_inputs_the_native_step_leaves_to_python(native, stub_dll, name):
    rig = Rig(native, stub_dll, 2)
    a = batch()
    wide = np.zeros((E, A, 2 * ACT), dtype=np.float32)
    bad = {"nested lists": a.tolist(), "float64": a.astype(np.float64), "int32": a.astype(np.int32), "strided slice": wide[:, :, ::2],
           "transposed": np.zeros((ACT, A, E), dtype=np.float32).T, "too few": a[1:], "too many": np.concatenate([a, a]), "not a buffer": object(),
           "big-endian": a.astype(">f4")}[name]
    assert rig.step(bad) is None
    assert (rig.stub.begin_calls, rig.stub.wait_calls, rig.env._cur, rig.errors) == (0, 0, 0, [])
    assert rig.step(a) is not None and rig.stub.last_set == 1          # and the next good batch steps as if nothing had been asked


def test_ring_states_the_native_step_leaves_to_python(native, stub_dll):
    rig = Rig(native, stub_dll, 2)                 # a ring of two that would have to grow: Python adds the set
    a = batch()
    r0, r1 = rig.step(a), rig.step(a)
    assert rig.step(a) is None and rig.stub.begin_calls == 2 and rig.env._cur == 0
    del r0, r1
    rig.env._cur = 7                               # (an index that is no set of the ring)
    assert rig.step(a) is None and rig.stub.begin_calls == 2
    rig.stepper.clear()                            # close(): nothing left to step into
    assert rig.stepper.n_sets == 0 and rig.step(a) is None


def test_library_failures_raise_through_check(native, stub_dll):
    rig = Rig(native, stub_dll, 2)
    a = batch()
    rig.stub.wait_rc = -1
    with pytest.raises(RuntimeError, match="ac_step_host_actions failed: stub"):
        rig.step(a)
    assert (rig.stub.begin_calls, rig.stub.wait_calls, rig.env._cur) == (1, 1, 1)      # the step ran: its set is the current one
    assert rig.errors == [(-1, "ac_step_host_actions")]
    rig.stub.wait_rc, rig.stub.begin_rc = 0, -1
    with pytest.raises(RuntimeError, match="ac_step_host_actions failed: stub"):
        rig.step(a)
    assert (rig.stub.begin_calls, rig.stub.wait_calls) == (2, 1)                       # no wait after a begin that failed
    rig.stub.begin_rc = 0
    assert not rig.stepper.held(0) and not rig.stepper.held(1)                         # the failed steps' results are gone
    assert rig.step(a) is not None


def test_another_thread_runs_while_the_wait_blocks(native, stub_dll):
    rig = Rig(native, stub_dll, 2)
    rig.stub.wait_ms = 50
    stamps, stop = [], threading.Event()

    def worker():
        while not stop.is_set():
            stamps.append(time.monotonic())        # (CLOCK_MONOTONIC, the stub's clock)

    t = threading.Thread(target=worker)
    t.start()
    try:
        assert rig.step(batch()) is not None
    finally:
        stop.set()
        t.join()
    t0, t1 = rig.stub.wait_t0, rig.stub.wait_t1
    assert t1 - t0 >= 0.049
    inside = sum(1 for s in stamps if t0 + 0.005 < s < t1 - 0.005)
    # a call that kept the GIL would leave this window empty; a free interpreter thread stamps it hundreds of thousands of times
    assert inside >= 1000, inside


@pytest.mark.parametrize("opt", ("-O1", "-O3"))
def test_set_picking_rule_under_the_sanitizers(tmp_path, opt):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "native_step_main"
    subprocess.check_call([cxx, "-std=c++17", opt, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "aircombat-selfplay_amd", "csrc"), os.path.join(ROOT, "tests", "host", "native_step_main.cpp"),
                           "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "native step pick checks ok" in run.stdout
