#!/usr/bin/env python3
"""Whole-ppo_update timings on one MI355X -> profiles/ppo_update_bench.txt ("The loss, the clip and Adam").

For each (N chunks, T) shape of tools/diag/act_train_bench.py and both head sets ([3, 5, 3] + [2, 2, 2, 2] with the shoot priors and
active_masks; [41, 41, 41, 30]) the tests' restated policy gets all three swaps (use_device_gru, use_device_mlp, use_device_act) and one
whole update is timed, from the on-device sample to the updated parameters, in two forms that alternate call by call within a run:

parent   the reference-form torch tail as the parent commit runs it: the loss in eager torch, zero_grad, backward, clip_grad_norm_
         twice with their .item(), optimizer.step(), and the four .item() calls train makes on the returned values;
device   DevicePPOTrainer.ppo_update: ppo_loss, zero_grad, backward, device_clip_adam_step, nothing read back.

Each run reports the median wall time per call (a host clock around the call and a synchronise) and the median device time (HIP events
around back-to-back calls); --runs consecutive runs are taken so the run-to-run spread is on the page. "after evaluate_actions" is the
parent leg minus a leg that stops at loss.backward() with no read-back: what the clip, the optimiser and the host waits add, which is
the share this change can remove. Then the two pieces alone at the same sizes, device against eager: the loss forward + backward on
[M, 1] inputs, and clip + Adam over the policy's own parameters with gradients in place.

    python tools/diag/ppo_update_bench.py [--reps 20] [--runs 3] [--out profiles/ppo_update_bench.txt] [--shapes 320x60,2400x8]
"""
import argparse
import copy
import os
import subprocess
import sys
import time
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aircombat_selfplay_amd as pkg  # noqa: E402
import act_train_util as U  # noqa: E402  (the tests' restatement of the reference's policy)
import mlp_train_util as MU  # noqa: E402
import ppo_update_util as PU  # noqa: E402  (the reference's loss, restated)

SHAPES = [(320, 60), (2400, 8), (4096, 60), (16384, 8)]
SPACES = [((3, 5, 3), 4), ((41, 41, 41, 30), 0)]
DONE = 0.02


def space_name(nvec, ns):
    return str(list(nvec)) + (f" + {[2] * ns}" if ns else "")


def timed(fns, reps, warm=3):
    """[(device ms, wall ms)] per function, the functions alternating call by call."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)] for _ in range(reps)]
    for e in ev:   # back to back: the only host waits are the functions' own
        e[0].record()
        for i, fn in enumerate(fns):
            fn(); e[i + 1].record()
    torch.cuda.synchronize()
    dev = [float(np.median([e[i].elapsed_time(e[i + 1]) for e in ev])) for i in range(len(fns))]
    wall = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); wall[i].append((time.perf_counter() - t0) * 1e3)
    return [(d, float(np.median(w))) for d, w in zip(dev, wall)]


class RefPolicy:
    """The reference PPOPolicy's surface over the restated actor and critic: evaluate_actions(obs, rnn_a, rnn_c, action, masks)."""

    def __init__(self, pol, active, kw):
        self.actor, self.critic, self.optimizer, self.active, self.kw = pol.actor, pol.critic, pol.optimizer, active, kw

    def evaluate_actions(self, obs, rnn_a, rnn_c, action, masks):
        logp, ent = self.actor.evaluate_actions(obs, rnn_a, action, masks, self.active, **self.kw)
        values, _ = self.critic(obs, rnn_c, masks)
        return values, logp, ent


def parent_update(policy, sample, args, read_back=True, tail=True):
    """The reference's ppo_update and the read-backs of its train, in torch, as the parent commit runs them."""
    obs, actions, masks, old_logp, adv, returns, vpreds, rnn_a, rnn_c = sample
    values, logp, ent = policy.evaluate_actions(obs, rnn_a, rnn_c, actions, masks)
    st = PU.loss_torch(dict(values=values, action_log_probs=logp, dist_entropy=ent, old_action_log_probs=old_logp, advantages=adv,
                            returns=returns, value_preds=vpreds), args.clip_param, args.value_loss_coef, args.entropy_coef)
    policy.optimizer.zero_grad()
    st["loss"].backward()
    if not tail:
        return
    an = nn.utils.clip_grad_norm_(policy.actor.parameters(), args.max_grad_norm).item()
    cn = nn.utils.clip_grad_norm_(policy.critic.parameters(), args.max_grad_norm).item()
    policy.optimizer.step()
    if read_back:
        return st["value_loss"].item(), st["policy_loss"].item(), st["policy_entropy_loss"].item(), an, cn, st["ratio"].item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_update_bench.txt"))
    ap.add_argument("--shapes", default="")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")] if a.shapes else SHAPES
    torch.manual_seed(0)
    args = PU.trainer_args()
    trainer = pkg.DevicePPOTrainer(args, torch.device("cuda", 0))
    lines = [f"# tools/diag/ppo_update_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, median of {a.reps} calls per run, "
             f"{a.runs} consecutive runs (ms): wall = per call with a synchronise, device = HIP events over back-to-back calls; the legs of a "
             f"comparison alternate call by call"]
    try:
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        if rev:
            lines.append(f"# parent commit {rev} plus the working tree of this change")
    except OSError:
        pass
    lines.append(f"{'N':>6} {'T':>3} {'what':72s} " + " ".join(f"{'wall' + str(r + 1):>8} {'dev' + str(r + 1):>8}" for r in range(a.runs)))

    def row(N, T, what, rs):
        lines.append(f"{N:6d} {T:3d} {what:72s} " + " ".join(f"{r[1]:8.3f} {r[0]:8.3f}" for r in rs))
        print(lines[-1], flush=True)

    def compare(N, T, names, fns, reps):
        runs = [timed(fns, reps) for _ in range(a.runs)]
        for i, name in enumerate(names):
            row(N, T, name, [r[i] for r in runs])
        return runs

    for N, T in shapes:
        M = N * T
        for nvec, ns in SPACES:
            g = torch.Generator(device="cuda").manual_seed(1)
            sizes = list(nvec) + [2] * ns
            act = torch.stack([torch.randint(0, n, (M,), device="cuda", generator=g) for n in sizes], -1).float()
            kw = {}
            if ns:
                pick = lambda vals: torch.tensor(vals, device="cuda")[torch.randint(0, 3, (M, 1), device="cuda", generator=g)]
                kw = {"alpha0": pick(U.ALPHA0), "beta0": pick(U.BETA0)}
            active = (torch.rand(M, 1, device="cuda", generator=g) > 0.1).float() if ns else None
            rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
            obs, ra, rc = rn(M, MU.OBS), rn(N, 1, 128), rn(N, 1, 128)
            masks = (torch.rand(M, 1, device="cuda", generator=g) > DONE).float()
            old_logp, adv, returns, vpreds = -2.0 + 0.1 * rn(M, 1), rn(M, 1), rn(M, 1), rn(M, 1)
            sample = (obs, act, masks, old_logp, adv, returns, vpreds, ra, rc)
            base = U.Policy(seed=3, nvec=nvec, ns=ns)
            assert pkg.use_device_gru(base) == 2 and pkg.use_device_mlp(base) == 4 and pkg.use_device_act(base) == 1
            legs = [RefPolicy(copy.deepcopy(base), active, kw) for _ in range(3)]
            name = space_name(nvec, ns)
            reps = max(5, a.reps // 2) if M > 100000 else a.reps
            runs = compare(N, T, [f"ppo_update {name}: parent (torch tail, 6 read-backs)", f"ppo_update {name}: device (DevicePPOTrainer)",
                                  f"ppo_update {name}: up to loss.backward() only, no read-back"],
                           [lambda: parent_update(legs[0], sample, args), lambda: trainer.ppo_update(legs[1], sample),
                            lambda: parent_update(legs[2], sample, args, tail=False)], reps)
            after = [(r[0][0] - r[2][0], r[0][1] - r[2][1]) for r in runs]
            row(N, T, f"ppo_update {name}: parent after evaluate_actions + backward (difference)", after)
            row(N, T, f"ppo_update {name}: device after evaluate_actions + backward (difference)", [(r[1][0] - r[2][0], r[1][1] - r[2][1]) for r in runs])
            # the pieces alone
            t = dict(values=rn(M, 1).requires_grad_(True), action_log_probs=(old_logp + 0.1 * rn(M, 1)).requires_grad_(True),
                     dist_entropy=rn(M, 1).abs().requires_grad_(True), old_action_log_probs=old_logp, advantages=adv, returns=returns, value_preds=vpreds)
            wrt = [t["values"], t["action_log_probs"], t["dist_entropy"]]

            def loss_device():
                loss, _ = pkg.ppo_loss(*wrt, old_logp, adv, returns, vpreds, clip_param=args.clip_param, value_loss_coef=args.value_loss_coef,
                                       entropy_coef=args.entropy_coef)
                torch.autograd.grad(loss, wrt)

            def loss_eager():
                torch.autograd.grad(PU.loss_torch(t, args.clip_param, args.value_loss_coef, args.entropy_coef)["loss"], wrt)

            if (nvec, ns) == SPACES[0]:   # the loss does not depend on the head set
                compare(N, T, ["loss forward + backward: device (ppo_loss)", "loss forward + backward: eager"], [loss_device, loss_eager], reps)
            pols = [legs[0], legs[1]]
            for p in pols:
                parent_update(p, sample, args, tail=False)   # gradients in place; both steps below rescale them in place, which times the same

            def step_device():
                pkg.device_clip_adam_step(pols[1].optimizer, args.max_grad_norm)

            def step_eager():
                nn.utils.clip_grad_norm_(pols[0].actor.parameters(), args.max_grad_norm).item()
                nn.utils.clip_grad_norm_(pols[0].critic.parameters(), args.max_grad_norm).item()
                pols[0].optimizer.step()

            compare(N, T, [f"clip + Adam {name}: device (device_clip_adam_step)", f"clip + Adam {name}: eager (2 x clip_grad_norm_.item(), step)"],
                    [step_device, step_eager], reps)
            del obs, act, masks, sample, t, wrt, legs, pols
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
