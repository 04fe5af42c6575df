#!/usr/bin/env python3
"""Where a VecEnv.step(numpy) of the headline config (or: <envs> <task> <per_side>) spends its time on the host: the action copy into the mapped buffer, the launch
call, the wait. (time.perf_counter_ns around the three pieces; ~0.1 us of timer overhead each.) Then VecEnv.step's own order -- header word,
doorbell, copy under the launch, wait (ac_step_host_actions) -- timed inside the library, with the kernel's retry counter, for the
library's share of the copy behind the doorbell or for every share of a comma-separated fourth argument. Last, VecEnv.step minus the
library's timers -- the time a step spends outside the library -- through ctypes and through the native entry (csrc/native_step.cpp)."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import aircombat_selfplay_amd as pkg

E = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
task = sys.argv[2] if len(sys.argv) > 2 else "singlecombat"
per_side = int(sys.argv[3]) if len(sys.argv) > 3 else 1
cfg = pkg.default_nvn_config(per_side, task=task) if per_side > 1 else pkg.default_config(task)
env = (pkg.HipShareVecEnv if cfg.n_agents > 2 else pkg.HipVecEnv)(cfg, E, seed=1)
env.reset()
rng = np.random.default_rng(0)
A = env.num_agents
acts = [np.concatenate([np.stack([rng.integers(0, n, size=(E, A)) for n in (41, 41, 41, 30)], axis=-1),
                        rng.random((E, A, env.act_dim - 4)) < 0.05], axis=-1).astype(np.float32) for _ in range(16)]
dll = env.lib.dll
h = env._h
now = time.perf_counter_ns
for label, do_copy in (("copy + launch + wait", True), ("launch + wait (actions left as they are)", False)):
    tc = tl = tw = 0
    K = 3000
    for it in range(K + 300):
        if it == 300:
            tc = tl = tw = 0
            T0 = now()
        cur = env._cur = env._cur ^ 1
        t0 = now()
        if do_copy:
            np.copyto(env._sets[cur]["actions"], acts[it & 15])
        t1 = now()
        dll.ac_step_host_async(h, cur)
        t2 = now()
        dll.ac_step_host_wait(h)
        t3 = now()
        tc += t1 - t0; tl += t2 - t1; tw += t3 - t2
    T1 = now()
    print(f"{label}: copy {tc / K / 1e3:.2f} us  launch call {tl / K / 1e3:.2f} us  wait {tw / K / 1e3:.2f} us   loop total {(T1 - T0) / K / 1e3:.2f} us/step")
# the same through VecEnv.step
t0 = now()
for it in range(3000):
    env.step(acts[it & 15])
print(f"VecEnv.step: {(now() - t0) / 3000 / 1e3:.2f} us/step")
# VecEnv.step through ac_step_host_actions, piece by piece as the library times them (ac_late_config's timing), for each share f of the
# batch copied behind the doorbell: the copy time hidden under the wait is `copy after`, and `retries` counts the row loads the kernel
# re-issued over the run (a path that retries in steady state is not one to ship). Fourth argument: the shares to sweep.
fractions = [float(x) for x in sys.argv[4].split(",")] if len(sys.argv) > 4 else [pkg.capi.AC_LATE_FRACTION_DEFAULT]
lib = env.lib


def late_pieces(env, f, label):
    """2000 timed steps at share f; returns (VecEnv.step, the sum of the library's four timers) in us per step"""
    h = env._h
    lib.check(lib.ac_late_config(h, f, -1, -1, 0), "ac_late_config")
    for it in range(300):
        env.step(acts[it & 15])
    before = pkg.capi.AcLateStats()
    lib.check(lib.ac_late_stats(h, C.byref(before)), "ac_late_stats")
    lib.check(lib.ac_late_config(h, -1.0, -1, -1, 1), "ac_late_config")
    K = 2000
    t0 = now()
    for it in range(K):
        env.step(acts[it & 15])
    dt = (now() - t0) / K / 1e3
    st = pkg.capi.AcLateStats()
    lib.check(lib.ac_late_stats(h, C.byref(st)), "ac_late_stats")
    lib.check(lib.ac_late_config(h, -1.0, -1, -1, 0), "ac_late_config")
    n = max(1, st.timed_steps - before.timed_steps)
    d = lambda name: (getattr(st, name) - getattr(before, name)) / n
    print(f"{label} f={f:.3f}: {st.steps - before.steps} late steps of {K}, retries {st.retries - before.retries} in {st.retry_steps - before.retry_steps} steps   "
          f"copy before {d('copy_before_us'):.2f} us  dispatch {d('dispatch_us'):.2f} us  copy after (under the wait) {d('copy_after_us'):.2f} us  "
          f"wait {d('wait_us'):.2f} us   VecEnv.step {dt:.2f} us/step")
    return dt, d("copy_before_us") + d("dispatch_us") + d("copy_after_us") + d("wait_us")


for f in fractions:
    late_pieces(env, f, "late actions")
env.close()
# VecEnv.step minus the library's own timers: what a step spends outside the library, through ctypes (AIRCOMBAT_NATIVE_STEP=0: set choice,
# checks, address, foreign call, result objects, all in the interpreter) and through the native entry (csrc/native_step.cpp; the figure
# still holds the result objects' construction, which now runs between the doorbell and the wait and shortens the wait by as much).
# Two passes each, alternating, so that a drift of the machine shows as a spread and not as a difference.
rows = {"ctypes": [], "native": []}
for rep in range(2):
    for path in ("ctypes", "native"):
        os.environ["AIRCOMBAT_NATIVE_STEP"] = "0" if path == "ctypes" else "1"
        e2 = (pkg.HipShareVecEnv if cfg.n_agents > 2 else pkg.HipVecEnv)(cfg, E, seed=1)
        if path == "native" and e2._native is None:
            print("outside the library, native path: the extension is not built here")
            e2.close()
            continue
        e2.reset()
        dt, inside = late_pieces(e2, fractions[-1], f"VecEnv.step through {path}")
        rows[path].append((dt, inside))
        e2.close()
for path, r in rows.items():
    if r:
        print(f"outside the library, {path} path: " + ", ".join(f"{dt:.2f} - {inside:.2f} = {dt - inside:.2f} us" for dt, inside in r))
