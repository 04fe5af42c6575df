#!/usr/bin/env python3
"""Device time of a whole-batch snapshot save / load and of clone_envs, against the 8 TB/s HBM peak.

Shapes: singlecombat at 4096 envs, 2v2 scenario_nvn hierarchical at 4096 envs, singlecombat at 2^19 envs (2^20 aircraft). Times are HIP
events recorded on the handle's own stream around `reps` back-to-back calls, after warm-up calls; one line per shape and operation.
Bytes moved: save / load = 2 x the snapshot size (read + write); clone of n envs = 2 x n x the per-env bytes. clone_envs and a partial
restore include their host-side index check (one host wait for the stream).

    python tools/diag/snapshot_bench.py [--reps 50]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PEAK = 8.0e12


def timed(torch, stream, fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import aircombat_selfplay_amd as pkg
    shapes = [("singlecombat", pkg.default_config("singlecombat"), 4096),
              ("scenario_nvn_2v2_hierarchical", pkg.default_nvn_config(2, task="scenario_nvn", hierarchical=True), 4096),
              ("singlecombat_2^20_aircraft", pkg.default_config("singlecombat"), 1 << 19)]
    for name, cfg, E in shapes:
        cls = pkg.HipShareVecEnv if cfg.n_agents > 2 else pkg.HipVecEnv
        env = cls(cfg, E, seed=1)
        env.reset()
        stream = torch.cuda.ExternalStream(env.lib.ac_stream(env._h))
        snap = env.snapshot()
        env.sync()
        size = snap.nbytes
        ptr = C.c_void_p(snap.data.data_ptr())
        t_save = timed(torch, stream, lambda: env.lib.check(env.lib.ac_snapshot_save(env._h, ptr), "ac_snapshot_save"), args.reps)
        t_load = timed(torch, stream, lambda: env.lib.check(env.lib.ac_snapshot_load(env._h, ptr), "ac_snapshot_load"), args.reps)
        per_env = (size - 1024) / E
        rows = [("save", t_save, 2 * size), ("load", t_load, 2 * size)]
        for n in (E // 4, E):
            src = np.zeros(n, dtype=np.int32)                     # one engagement into n envs (a source repeated: legal)
            dst = np.arange(n, dtype=np.int32)
            dsrc = torch.from_numpy(src).cuda()
            ddst = torch.from_numpy(dst).cuda()
            t = timed(torch, stream, lambda: env.lib.check(env.lib.ac_clone_envs(env._h, C.c_void_p(dsrc.data_ptr()), C.c_void_p(ddst.data_ptr()), n),
                                                          "ac_clone_envs"), args.reps)
            rows.append((f"clone_envs n={n}", t, 2 * n * per_env))
        for label, t, nbytes in rows:
            print(json.dumps({"shape": name, "envs": E, "aircraft": E * cfg.n_agents, "op": label, "snapshot_bytes": size,
                              "us": round(t * 1e6, 2), "GB_s": round(nbytes / t / 1e9, 1), "of_peak": round(nbytes / t / PEAK, 3)}))
        env.close()
        del snap


if __name__ == "__main__":
    main()
