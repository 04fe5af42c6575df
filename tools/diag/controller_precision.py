#!/usr/bin/env python3
"""The low-level controller's two forms side by side in ONE process on one device (interleaved rounds): the fast form (two fp16 pieces per
value, AC_CTL_FAST, the default) and the reference-precision form (three bf16 pieces, AC_CTL_FP32), each with the default workgroup shape,
at the three batches the as-shipped configs call it with: 8192 aircraft (scenario1), 16 384 (2v2), 32 768 (4v4). HIP events around the
controller kernel and the step kernel of every device-resident step (ac_step_timed_device). Writes profiles/controller_precision.txt."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import aircombat_selfplay_amd as pkg

E = 4096
ROUNDS, STEPS = 5, 200
cases = [("scenario1", 1), ("scenario_nvn", 2), ("scenario_nvn", 4)]
FORMS = ("fast", "fp32")
os.environ.pop("AIRCOMBAT_CTL_PRECISION", None)
os.environ.pop("AIRCOMBAT_CTL_ROWS", None)
rng = np.random.default_rng(0)
lines = [f"device: {torch.cuda.get_device_name(0)}; {E} envs, {ROUNDS} interleaved rounds x {STEPS} device-resident steps per form, medians"]
for task, per_side in cases:
    envs = {}
    for form in FORMS:
        cfg = pkg.default_config(task, hierarchical=True) if per_side == 1 else pkg.default_nvn_config(per_side, task=task, hierarchical=True)
        cls = pkg.HipShareVecEnv if cfg.n_agents > 2 else pkg.HipVecEnv
        envs[form] = cls(cfg, E, seed=1, copy=False, controller_precision=form)
        assert envs[form].controller_precision == form
        envs[form].reset()
    A = envs["fast"].num_agents
    pool = []
    for _ in range(8):
        a = np.stack([rng.integers(0, n, size=(E, A)) for n in (3, 5, 3)], axis=-1).astype(np.float32)
        a = np.concatenate([a, (rng.random((E, A, envs["fast"].act_dim - 3)) < 0.05).astype(np.float32)], axis=-1)
        pool.append(torch.from_numpy(a).cuda())
    ptrs = [t.data_ptr() for t in pool]
    res = {f: [] for f in FORMS}
    ctl, stp = C.c_float(), C.c_float()
    for r in range(ROUNDS + 1):
        for form in FORMS:
            env = envs[form]
            tc = ts = 0.0
            for i in range(STEPS):
                env.lib.check(env.lib.ac_step_timed_device(env._h, ptrs[i % 8], C.byref(ctl), C.byref(stp)), "ac_step_timed_device")
                tc += ctl.value; ts += stp.value
            if r:
                res[form].append((tc / STEPS * 1e3, ts / STEPS * 1e3))
    med = {}
    for form in FORMS:
        c = sorted(x[0] for x in res[form]); s = sorted(x[1] for x in res[form])
        med[form] = c[len(c) // 2]
        lines.append(f"{task} x{per_side} ({E * A:5d} aircraft) {form:4s}: controller median {c[len(c) // 2]:6.2f} us (min {c[0]:6.2f})   "
                     f"step kernel median {s[len(s) // 2]:6.2f} us")
    lines.append(f"    fp32 / fast controller time: {med['fp32'] / med['fast']:.2f}x")
    for env in envs.values():
        env.close()
    print("\n".join(lines[-3:]), flush=True)
out = os.path.join(ROOT, "profiles", "controller_precision.txt")
os.makedirs(os.path.dirname(out), exist_ok=True)
open(out, "w").write("\n".join(lines) + "\n")
