#!/usr/bin/env python3
"""Diagnostic: free-flight (open-loop) difference between the fp32 HIP step and the float64 oracle — no state injection at all.

Both start from the same initial conditions and take the same action sequence. Per env step it records, over all aircraft, the
position difference (NEU, m), the attitude difference (roll / pitch / yaw, rad), the velocity difference (m/s), the observation and
reward differences, the munition differences while closing, and whether the discrete decisions agree (flight control system switches,
turbine phase word, status, weapon bookkeeping, munition status / target / model). Writes <out>/open_loop_<mode>_<form>.json: the
curves the frozen envelopes of tests/test_gpu_open_loop.py were taken from, and the per-form table of DESIGN.md section 8.

usage: open_loop.py straight|random [steps] [envs] [form] [twin] [out=DIR]
    out=DIR: where the JSON goes (default: diag_out/ in the repository root)
    form: an index into open_loop_util.RANDOM_FORMS or one of its ids (default 0, the C2 three-wave form); its environment pins are set here
    twin: compare the oracle's fp32 twin (tests/test_open_loop_twin.py) instead of the device: no GPU needed"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from open_loop_util import RANDOM_FORM_IDS, RANDOM_FORMS, Fp32Twin, OpenLoopPair, OracleSide, envelope, random_actions  # noqa: E402


def main():
    out_dir = os.path.join(ROOT, "diag_out")
    for a in [a for a in sys.argv if a.startswith("out=")]:
        out_dir = os.path.abspath(a[4:])
        sys.argv.remove(a)
    mode = sys.argv[1] if len(sys.argv) > 1 else "straight"
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 600
    E = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    form = sys.argv[4] if len(sys.argv) > 4 else "0"
    twin = len(sys.argv) > 5 and sys.argv[5] == "twin"
    fi = int(form) if form.isdigit() else RANDOM_FORM_IDS.index(form)
    name, task, per_side, pins, _, seed = RANDOM_FORMS[fi]
    os.environ.update(pins)         # before the package creates a handle: ac_create reads them
    import aircombat_selfplay_amd as pkg
    from oracle import oracle
    sides = None
    if twin:
        def sides(cfg, ocfg, per, ix):
            return Fp32Twin(oracle, ocfg, per, ix), OracleSide(oracle, ocfg, per, ix)
    pair = OpenLoopPair(pkg, oracle, E, spread=True, task=task, per_side=per_side, sides=sides)
    E = pair.E
    rows = []
    age = np.zeros(E, dtype=np.int64)
    actions = random_actions(task, E, pair.A, steps, seed) if mode == "random" else (pair.straight_action() for _ in range(steps))
    worst = {}
    for step, act in enumerate(actions):
        m = pair.step(act)
        live = m["live"]
        age += 1
        env = envelope(age)
        row = {"step": step + 1, "live_envs": int(live.sum()), "max_age": int(age.max())}
        for k in ("pos_m", "att_rad", "vel_ms", "obs", "rew"):
            v = m[k][live]
            row[k + "_max"] = float(v.max()) if v.size else None
            row[k + "_p50"] = float(np.median(v)) if v.size else None
            if v.size:
                row[k + "_age_of_max"] = int(age[live][np.unravel_index(v.argmax(), v.shape)[0]])
                worst[k] = max(worst.get(k, 0.0), float((m[k] / (8.0 * env[k][:, None]))[live].max()))
        for k in ("msl_pos_m", "msl_vel_ms"):
            row[k + "_max"] = float(m[k][live].max()) if live.any() else None
        age[pair.last_reset] = 0
        rows.append(row)
        if (step + 1) % 50 == 0:
            print(row, flush=True)
    out = {"mode": mode, "form": name, "twin": twin, "envs": E, "steps": steps, "rows": rows, "horizon_steps": pair.horizon.tolist(),
           "horizon_reason": pair.reason, "done_mismatch_envs": int(pair.done_mismatch.sum()), "unexplained": [repr(u) for u in pair.unexplained],
           "worst_fraction_of_8x_envelope": worst, "munitions": pair.worst_msl, "munitions_flown": pair.msl_flown, "munitions_ended": pair.msl_ended,
           "envs_with_a_munition": int(pair.flown.sum())}
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"open_loop_{mode}_{RANDOM_FORM_IDS[fi]}{'_twin' if twin else ''}.json"), "w") as f:
        json.dump(out, f)
    h = pair.horizon
    r3 = lambda d: {k: round(v, 3) for k, v in d.items()}
    print(f"{mode} [{name}{', fp32 twin' if twin else ''}]: horizon (first step a discrete decision differs) min {h.min()} p10 {np.percentile(h, 10):.0f} "
          f"median {np.median(h):.0f} never {int((h >= steps).sum())}/{E}; reasons {pair.reason_counts()}; unexplained {len(pair.unexplained)}; fraction of the 8x "
          f"envelope used: aircraft {r3(worst)}, munitions closing {r3(pair.worst_msl['closing'])}, after the pass {r3(pair.worst_msl['after the pass'])}; "
          f"munitions flown {pair.msl_flown} in {int(pair.flown.sum())}/{E} envs, ended {pair.msl_ended}")
    pair.close()


if __name__ == "__main__":
    main()
