"""The stream-ordered hand-over's host side (include/aircombat_epoch.h, csrc/epoch_gather.hpp), no GPU: where the fields of an epoch
lie in the flat array, the refusals that need no handle, the kernel's row function with its clamp, the exports."""
import ctypes as C
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("obs", "share_obs", "actions", "masks", "active_masks", "action_log_probs", "advantages", "returns", "value_preds",
         "rnn_states_actor", "rnn_states_critic")
# (T, E, A, L, n_mb, share_obs_dim): the shapes of tests/test_gpu_epoch.py, for both buffer classes
SHAPES = [(7, 3, 2, 4, 2, 42), (5, 2, 1, 1, 3, 42), (8, 4, 2, 8, 1, 42), (64, 33, 2, 8, 5, 42), (64, 33, 2, 8, 5, 43), (64, 33, 2, 8, 5, 44)]


def capi_of(pkg):
    """The bindings module the loaded library's signatures were made from (``pkg.capi`` may be a second import of it under the alias name)."""
    return importlib.import_module("aircombat-selfplay_amd.capi")


def config(pkg, T, E, A, share):
    return capi_of(pkg).AcBufferConfig(T, E, A, 21, share, 7, 7 if share else 1, 1, 128, 1, 0, 0.99, 0.95)


def layout(pkg, cfg, n_mb, mb, L):
    off, total = (C.c_int64 * 11)(), C.c_int64(-7)
    rc = pkg.load_library().ac_buffer_epoch_layout_for(C.byref(cfg), n_mb, mb, L, off, C.byref(total))
    return rc, list(off), total.value


@pytest.mark.parametrize("shared", [False, True], ids=["ppo", "shared"])
@pytest.mark.parametrize("T,E,A,L,n_mb,share", SHAPES)
def test_layout_is_aligned_disjoint_and_complete(pkg, T, E, A, L, n_mb, share, shared):
    share = share if shared else 0
    mb = (E * T // L) // n_mb
    rc, off, total = layout(pkg, config(pkg, T, E, A, share), n_mb, mb, L)
    assert rc == 0
    dims = dict(zip(NAMES, (21, share, 7, 1, 1 if shared else 0, 7 if shared else 1, 1, 1, 1, 128, 128)))
    spans, padded = [], 0
    for name, o in zip(NAMES, off):
        if dims[name] == 0:
            assert o == -1, name                       # a field this buffer lacks
            continue
        rows = mb if name.startswith("rnn") else L * mb
        size = n_mb * rows * dims[name]
        assert o >= 0 and o % 4 == 0, (name, o)        # every field starts at a multiple of 4 floats
        spans.append((o, o + size))
        padded += -(-size // 4) * 4
    spans.sort()
    assert spans[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= total   # no overlap, all inside
    assert total == padded                             # the fields' sizes plus the padding to 4 floats, nothing else
    assert [o for o in off if o >= 0] == sorted(o for o in off if o >= 0)   # in the order of ac_buffer_batch_t


def test_refusals_without_a_handle(pkg):
    lib = pkg.load_library()
    cfg = config(pkg, 7, 3, 2, 0)
    off, total = (C.c_int64 * 11)(), C.c_int64()
    for call, what in ((lambda: lib.ac_buffer_epoch_layout_for(None, 2, 2, 4, off, C.byref(total)), "null argument"),
                       (lambda: lib.ac_buffer_epoch_layout_for(C.byref(cfg), 2, 2, 4, None, C.byref(total)), "null argument"),
                       (lambda: lib.ac_buffer_epoch_layout_for(C.byref(cfg), 2, 2, 4, off, None), "null argument"),
                       (lambda: lib.ac_buffer_epoch_layout(None, 2, 2, 4, off, C.byref(total)), "null argument"),
                       (lambda: lib.ac_buffer_epoch_layout_for(C.byref(cfg), 0, 2, 4, off, C.byref(total)), "must be positive"),
                       (lambda: lib.ac_buffer_epoch_layout_for(C.byref(cfg), 2, -1, 4, off, C.byref(total)), "must be positive"),
                       (lambda: lib.ac_buffer_epoch_layout_for(C.byref(cfg), 2, 2, 0, off, C.byref(total)), "must be positive"),
                       # T * N = 42 rows: 2 * 5 * 4 = 40 fit, 2 * 6 * 4 = 48 and 3 * 4 * 4 = 48 do not; nor does a product past 2^63
                       (lambda: lib.ac_buffer_epoch_layout_for(C.byref(cfg), 2, 6, 4, off, C.byref(total)), "exceeds the buffer"),
                       (lambda: lib.ac_buffer_epoch_layout_for(C.byref(cfg), 3, 4, 4, off, C.byref(total)), "exceeds the buffer"),
                       (lambda: lib.ac_buffer_epoch_layout_for(C.byref(cfg), 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, off, C.byref(total)), "exceeds the buffer"),
                       (lambda: lib.ac_buffer_gather_epoch(None, None, 8, 2, 2, 4, 8), "null argument"),
                       (lambda: lib.ac_buffer_compute_returns_on(None, None, 8), "null argument"),
                       (lambda: lib.ac_buffer_advantages_on(None, None), "null handle")):
        assert call() == -1
        assert what in lib.last_error(), (what, lib.last_error())
    assert lib.ac_buffer_epoch_layout_for(C.byref(cfg), 2, 5, 4, off, C.byref(total)) == 0
    bad = config(pkg, 7, 3, 2, 0)
    bad.obs_dim = 0
    assert lib.ac_buffer_epoch_layout_for(C.byref(bad), 2, 2, 4, off, C.byref(total)) == -1 and "sizes must be positive" in lib.last_error()


@pytest.mark.parametrize("T,N,L", [(7, 6, 4), (5, 2, 1), (8, 8, 8), (64, 66, 8), (3, 5, 7)])
def test_row_function_and_its_clamp(pkg, T, N, L):
    """source row = t * N + col with row = chunk * L + l, col = row // T, t = row % T; an index outside [0, T * N // L - 1] is clamped to
    the nearest valid chunk, so that no index can name a row outside the arrays (memory safety, not validation)."""
    f = pkg.load_library().ac_buffer_epoch_source_row_host
    n_chunks = T * N // L
    want = lambda c, l: ((c * L + l) % T) * N + (c * L + l) // T
    seen = set()
    for c in range(n_chunks):
        for l in range(L):
            got = f(c, l, L, T, N)
            assert got == want(c, l) and 0 <= got < T * N, (c, l, got)
            seen.add(got)
    assert len(seen) == n_chunks * L                 # distinct rows: the chunks tile the sequence view
    for bad, to in ((-1, 0), (-2 ** 31, 0), (n_chunks, n_chunks - 1), (n_chunks + 5, n_chunks - 1), (2 ** 31 - 1, n_chunks - 1)):
        for l in (0, L - 1):
            assert f(bad, l, L, T, N) == want(to, l), (bad, l)
    lib = pkg.load_library()
    for a in ((0, L, L, T, N), (0, -1, L, T, N), (0, 0, 0, T, N), (0, 0, L, 0, N), (0, 0, L, T, 0), (0, 0, T * N + 1, T, N)):
        assert f(*a) == -1 and "ac_buffer_epoch_source_row_host" in lib.last_error()


def test_header_and_bindings_agree(pkg, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "aircombat_epoch.h")).read()
    declared = set(re.findall(r"\b(ac_buffer_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"ac_buffer_compute_returns_on", "ac_buffer_advantages_on", "ac_buffer_epoch_layout", "ac_buffer_epoch_layout_for",
                        "ac_buffer_gather_epoch", "ac_buffer_epoch_source_row_host"}
    lib, capi = pkg.load_library(), capi_of(pkg)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib.path], text=True)
    for sym in declared:
        assert sym in capi.SIGNATURES and hasattr(lib, sym) and re.search(rf"\bT {sym}\b", exported), sym
    # the header adds no struct of its own; the one it takes and its field count must be what ctypes passes
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "aircombat_epoch.h"\n'
                   'int main(){printf("%zu %d %zu", sizeof(ac_buffer_config_t), (int)AC_EPOCH_NFIELDS, sizeof(ac_buffer_batch_t) / sizeof(float*));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a, n, members = map(int, subprocess.check_output([str(exe)], text=True).split())
    assert a == C.sizeof(capi.AcBufferConfig) and n == capi.AC_EPOCH_NFIELDS == members == 11
    assert capi.AC_EPOCH_FIELDS == tuple(name for name, _ in capi.AcBufferBatch._fields_) == NAMES


def test_exports(pkg):
    assert pkg.DeviceEpoch.__name__ == "DeviceEpoch" and "DeviceEpoch" in pkg.__all__
    for name in ("epoch", "queue_advantages"):
        assert callable(getattr(pkg.DeviceReplayBuffer, name)) and getattr(pkg.DeviceSharedReplayBuffer, name) is getattr(pkg.DeviceReplayBuffer, name)
    e = pkg.DeviceEpoch("flat", "order", [(1, 2), (3, 4)], ("a", "b"))
    assert len(e) == 2 and e[1] == (3, 4) and list(e) == [(1, 2), (3, 4)] and e.order == "order"
    import inspect
    assert inspect.signature(pkg.DeviceReplayBuffer.compute_returns).parameters["wait"].default is True
    assert inspect.signature(pkg.DeviceRollout.compute_returns).parameters["wait"].default is True
    train = inspect.signature(pkg.DevicePPOTrainer.train).parameters
    assert train["stream_ordered"].default is None and train["chunk_orders"].default is None
