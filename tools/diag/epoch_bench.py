#!/usr/bin/env python3
"""The rollout buffer's hand-over to the update, blocking against stream-ordered, on one MI355X -> profiles/epoch_bench.txt
("Stream-ordered training data").

Two shapes: "reference" = the reference's own training shape, 32 envs x 3000 steps, chunks of 60, 5 minibatches, 4 epochs; "wide" =
4096 envs x 64 steps, chunks of 8, 5 minibatches, 4 epochs. Per shape:

(a) the gather: the 20 ``minibatch(on_device=True)`` calls of a train (with ``ac_buffer_advantages`` once per epoch, as the generator runs
    it) against 4 ``epoch`` calls, for the PPO buffer (obs 21, actions 7) and the shared one (2 agents, share_obs 42). Wall time: a host
    clock around the calls and one synchronise at the end, the two legs alternating, median per run. Kernel time: the gather kernels'
    durations summed by ``rocprofv3 --kernel-trace --stats`` in runs of their own (one child process per leg, the profiler off
    everywhere else). Bytes: every gathered float once read and once written, from the shapes; over the kernel time, as a share of
    the 8.0 TB/s HBM peak. The buffers here fit the 256 MiB Infinity Cache, so that share says how far the gather is from the
    memory system's best, not that HBM is what it waits for.
(b) a whole ``DevicePPOTrainer.train`` on the tests' restated policy with the three swaps (use_device_gru, use_device_mlp,
    use_device_act): the default path against ``stream_ordered=True``, alternating call by call, wall time with a synchronise, and the
    time the call itself takes to return (how far the host runs ahead); and every kernel's duration summed over a train, each leg
    traced in a run of its own.
(c) the default ``train`` and one ``minibatch`` call with this tree's library and, with ``--parent-root``, with a checkout of the
    parent commit built in that directory: the paths this change leaves alone. Each tree is measured in two processes, the trees
    alternating; the margin is the parent's own spread from run to run and from process to process.

Every measurement is a child process of its own under a time limit; the first one that fails ends the run. ``--runs`` consecutive runs
are on the page so that the spread is.

    python tools/diag/epoch_bench.py [--runs 3] [--reps 10] [--shapes reference,wide] [--parent-root DIR] [--no-kernel-stats]
"""
import argparse
import csv
import glob
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = {"reference": dict(E=32, T=3000, L=60, n_mb=5, epochs=4), "wide": dict(E=4096, T=64, L=8, n_mb=5, epochs=4)}
OBS, ACT, SHARE, HIDDEN = 21, 7, 42, 128
HBM_PEAK = 8.0e12
GATHER_KERNELS = {"minibatch": "gather_rows_kernel", "epoch": "epoch_gather_kernel"}


def buffer_args(s):
    return types.SimpleNamespace(buffer_size=s["T"], n_rollout_threads=s["E"], gamma=0.99, use_proper_time_limits=False, use_gae=True, gae_lambda=0.95,
                                 recurrent_hidden_size=HIDDEN, recurrent_hidden_layers=1)


def gathered_bytes(s, shared):
    """Bytes the gather of one epoch has to move: each float of each minibatch read once and written once, plus the chunk indices."""
    chunks = s["E"] * s["T"] // s["L"]
    used = chunks // s["n_mb"] * s["n_mb"]
    per_step = OBS + ACT + 1 + (ACT if shared else 1) + 3 + ((SHARE + 1) if shared else 0)
    return 2 * 4 * (used * s["L"] * per_step + used * 2 * HIDDEN) + 4 * used


# ---- the children
def child_setup(root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import torch
    torch.cuda.init()
    import aircombat_selfplay_amd as pkg
    return torch, pkg


def make_buffer(torch, pkg, s, shared, obs=OBS, act=ACT, share=SHARE, seed=1):
    a = buffer_args(s)
    buf = pkg.DeviceSharedReplayBuffer(a, 2, obs, share, act) if shared else pkg.DeviceReplayBuffer(a, 1, obs, act)
    g = torch.Generator(device="cuda").manual_seed(seed)
    for name in ("obs", "rewards", "action_log_probs", "value_preds", "rnn_states_actor", "rnn_states_critic") + (("share_obs",) if shared else ()):
        buf.device_tensor(name).normal_(generator=g)
    buf.device_tensor("action_log_probs").mul_(0.1).sub_(2.0)
    m = buf.device_tensor("masks")
    m.copy_((torch.rand(m.shape, device="cuda", generator=g) > 0.02).float())
    nv = torch.randn(s["E"] * buf.num_agents, device="cuda", generator=g)
    torch.cuda.synchronize()
    buf.compute_returns(nv, on_device=True)
    return buf


def gather_legs(torch, buf, s, orders):
    n_mb, L = s["n_mb"], s["L"]
    mb = len(orders[0]) // n_mb

    def minibatches():
        for o in orders:
            buf.lib.ac_buffer_advantages(buf._h)       # once per epoch, as recurrent_generator does
            for i in range(n_mb):
                buf.minibatch(o[i * mb:(i + 1) * mb], L, on_device=True)

    def epochs():
        return [buf.epoch(n_mb, L, chunk_order=o) for o in orders]
    return {"minibatch": minibatches, "epoch": epochs}


def alternate(torch, fns, reps, warm=2):
    """name -> (median wall ms with a synchronise, median ms until the call returned), the functions alternating call by call."""
    import numpy as np
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    wall, back = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter(); keep = fn(); t1 = time.perf_counter(); torch.cuda.synchronize(); t2 = time.perf_counter()
            del keep
            wall[k].append((t2 - t0) * 1e3); back[k].append((t1 - t0) * 1e3)
    return {k: (float(np.median(wall[k])), float(np.median(back[k]))) for k in fns}


def orders_for(s, n):
    import numpy as np
    return [np.random.default_rng(e).permutation(s["E"] * s["T"] // s["L"]) for e in range(n)]


def child_gather(a):
    torch, pkg = child_setup(a.root)
    s = SHAPES[a.shape]
    out = {}
    for shared in (False, True):
        buf = make_buffer(torch, pkg, s, shared)
        legs = gather_legs(torch, buf, s, orders_for(s, s["epochs"]))
        out["shared" if shared else "ppo"] = [alternate(torch, legs, a.reps) for _ in range(a.runs)]
        buf.close()
    print("RESULT " + json.dumps(out))


def child_trace(a):
    """One leg of (a), a.reps times after a warm-up, for the profiler: both buffer classes in turn."""
    torch, pkg = child_setup(a.root)
    s = SHAPES[a.shape]
    for shared in (False, True):
        buf = make_buffer(torch, pkg, s, shared)
        fn = gather_legs(torch, buf, s, orders_for(s, s["epochs"]))[a.which]
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        buf.close()
    print("RESULT " + json.dumps({"calls": a.reps * s["epochs"]}))


def restated_policy(torch, pkg):
    import act_train_util as AU
    G = importlib.import_module("aircombat-selfplay_amd.gru_train")
    M = importlib.import_module("aircombat-selfplay_amd.mlp_train")
    A = importlib.import_module("aircombat-selfplay_amd.act_train")
    pol = AU.Policy(seed=3)
    assert G.use_device_gru(pol) == 2 and M.use_device_mlp(pol) == 4 and A.use_device_act(pol) == 1
    return types.SimpleNamespace(actor=pol.actor, critic=pol.critic, optimizer=pol.optimizer,
                                 evaluate_actions=lambda obs, ra, rc, act, m: pol.evaluate_actions(obs, obs, ra, rc, act, m))


def trainer_for(torch, pkg, s):
    import ppo_update_util as PU
    Pu = importlib.import_module("aircombat-selfplay_amd.ppo_update")
    return Pu.DevicePPOTrainer(PU.trainer_args(ppo_epoch=s["epochs"], num_mini_batch=s["n_mb"], data_chunk_length=s["L"]), torch.device("cuda", 0))


def train_buffer(torch, pkg, s):
    import mlp_train_util as MU
    buf = make_buffer(torch, pkg, s, False, obs=MU.OBS, act=len(MU.NVEC))
    g = torch.Generator(device="cuda").manual_seed(2)
    acts = buf.device_tensor("actions")
    for i, n in enumerate(MU.NVEC):
        acts[..., i] = torch.randint(0, n, acts[..., i].shape, device="cuda", generator=g).float()
    torch.cuda.synchronize()
    return buf


def child_train(a):
    torch, pkg = child_setup(a.root)
    s = SHAPES[a.shape]
    buf, tr = train_buffer(torch, pkg, s), trainer_for(torch, pkg, s)
    orders = orders_for(s, s["epochs"])
    pols = {k: restated_policy(torch, pkg) for k in ("default", "stream_ordered")}
    legs = {"default": lambda: tr.train(pols["default"], buf, chunk_orders=orders),
            "stream_ordered": lambda: tr.train(pols["stream_ordered"], buf, chunk_orders=orders, stream_ordered=True)}
    print("RESULT " + json.dumps([alternate(torch, legs, a.reps) for _ in range(a.runs)]))


def child_trace_train(a):
    """One leg of (b), a.reps times after a warm-up, for the profiler."""
    torch, pkg = child_setup(a.root)
    s = SHAPES[a.shape]
    buf, tr, pol = train_buffer(torch, pkg, s), trainer_for(torch, pkg, s), restated_policy(torch, pkg)
    orders = orders_for(s, s["epochs"])
    for _ in range(a.reps):
        tr.train(pol, buf, chunk_orders=orders, stream_ordered=a.which == "stream_ordered")
    torch.cuda.synchronize()
    print("RESULT " + json.dumps({"calls": a.reps}))


def child_untouched(a):
    """(c): the default train and one minibatch call with the package of a.root (this tree, or a built checkout of the parent)."""
    torch, pkg = child_setup(a.root)
    s = SHAPES[a.shape]
    buf, tr = train_buffer(torch, pkg, s), trainer_for(torch, pkg, s)
    orders = orders_for(s, s["epochs"])
    pol = restated_policy(torch, pkg)
    mb = len(orders[0]) // s["n_mb"]
    buf.lib.ac_buffer_advantages(buf._h)
    legs = {"train": lambda: tr.train(pol, buf, chunk_orders=orders), "minibatch": lambda: buf.minibatch(orders[0][:mb], s["L"], on_device=True)}
    print("RESULT " + json.dumps([alternate(torch, legs, a.reps) for _ in range(a.runs)]))


CHILDREN = {"gather": child_gather, "trace": child_trace, "train": child_train, "trace_train": child_trace_train, "untouched": child_untouched}


# ---- the parent process: never touches the GPU itself
def run_child(argv, limit, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__)] + argv
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"epoch_bench: child {' '.join(argv)} ended with {p.returncode}; nothing more is started")
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise SystemExit(f"epoch_bench: child {' '.join(argv)} printed no result")


def all_kernels_ns(stats_dir):
    """(total ns, launches) of every kernel in rocprofv3's kernel stats, and the five largest as (name, ns, launches)."""
    rows = []
    for path in glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True):
        rows += [(r["Name"], int(float(r["TotalDurationNs"])), int(r["Calls"])) for r in csv.DictReader(open(path))]
    rows.sort(key=lambda r: -r[1])
    return sum(r[1] for r in rows), sum(r[2] for r in rows), rows[:5]


def kernel_ns(stats_dir, needle):
    """(total ns, calls) of the kernels whose name holds `needle` in rocprofv3's kernel stats."""
    total, calls = 0, 0
    for path in glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if needle in r["Name"]:
                total += int(float(r["TotalDurationNs"])); calls += int(r["Calls"])
    return total, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="reference,wide")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epoch_bench.txt"))
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--no-kernel-stats", action="store_true")
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    ap.add_argument("--child", default="")
    ap.add_argument("--shape", default="reference")
    ap.add_argument("--which", default="epoch")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return CHILDREN[a.child](a)
    lines = [f"# tools/diag/epoch_bench.py: {a.runs} consecutive runs, each the median of {a.reps} calls (ms); the legs of a comparison alternate call",
             "# by call. wall = host clock around the calls and a synchronise; returned = until the calls came back to the host.",
             "# kernel = the gather kernels' summed durations per train (4 epochs), rocprofv3 --kernel-trace --stats, a run of its own per leg."]
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    if rev:
        lines.append(f"# parent commit {rev} plus the working tree of this change")

    def say(text):
        lines.append(text)
        print(text, flush=True)

    common = ["--runs", str(a.runs), "--reps", str(a.reps)]
    for shape in a.shapes.split(","):
        s = SHAPES[shape]
        say(f"\n== {shape}: {s['E']} envs x {s['T']} steps, chunks of {s['L']}, {s['n_mb']} minibatches, {s['epochs']} epochs")
        res = run_child(["--child", "gather", "--shape", shape] + common, a.limit)
        kern = {}
        if not a.no_kernel_stats:
            for which, needle in GATHER_KERNELS.items():
                with tempfile.TemporaryDirectory() as tmp:
                    done = run_child(["--child", "trace", "--shape", shape, "--which", which, "--reps", "3"], a.limit,
                                     prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "stats", "--"])
                    ns, calls = kernel_ns(tmp, needle)
                    kern[which] = (ns / 3 / 2, calls)      # per train of one buffer class: 3 repetitions, 2 classes (summed: see below)
        say("(a) the gather of one train: 20 minibatch(on_device=True) calls against 4 epoch calls")
        for cls in ("ppo", "shared"):
            for leg, label in (("minibatch", "20 x minibatch + 4 x advantages (blocking)"), ("epoch", "4 x epoch (stream-ordered)")):
                say(f"  {cls:6s} {label:44s} " + " ".join(f"wall {r[leg][0]:8.3f} returned {r[leg][1]:8.3f}" for r in res[cls]))
        if kern:
            byts = (gathered_bytes(s, False) + gathered_bytes(s, True)) / 2 * s["epochs"]
            for leg in ("minibatch", "epoch"):
                ns, calls = kern[leg]
                say(f"  kernel time per train, mean of the two classes: {leg:9s} {ns / 1e6:8.3f} ms in {calls // 6} launches per class and train; "
                    f"{byts / 1e6:.1f} MB gathered -> {byts / (ns * 1e-9) / 1e12:6.3f} TB/s = {100 * byts / (ns * 1e-9) / HBM_PEAK:5.1f} % of the 8.0 TB/s HBM peak")
        res = run_child(["--child", "train", "--shape", shape] + common, a.limit)
        say("(b) DevicePPOTrainer.train, the restated policy with the three swaps (PPO buffer, obs 12)")
        for leg in ("default", "stream_ordered"):
            say(f"  {leg:51s} " + " ".join(f"wall {r[leg][0]:8.3f} returned {r[leg][1]:8.3f}" for r in res))
        if not a.no_kernel_stats:
            for leg in ("default", "stream_ordered"):
                with tempfile.TemporaryDirectory() as tmp:
                    run_child(["--child", "trace_train", "--shape", shape, "--which", leg, "--reps", "4"], a.limit,
                              prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "stats", "--"])
                    ns, calls, top = all_kernels_ns(tmp)
                say(f"  {leg:15s} kernel time per train (all kernels, 4 trains traced, the first one cold) {ns / 4e6:8.3f} ms in {calls // 4} launches; largest: "
                    + "; ".join(f"{n.split('(')[0][-48:]} {t / 4e6:.3f}" for n, t, _ in top))
        say("(c) the untouched paths: default train and one minibatch(on_device=True) call; a process per line, the two trees alternating")
        roots = [("this tree", ROOT)] + ([("parent commit", os.path.abspath(a.parent_root))] if a.parent_root else [])
        for name, root in roots * 2:
            res = run_child(["--child", "untouched", "--shape", shape, "--root", root] + common, a.limit)
            for leg in ("train", "minibatch"):
                say(f"  {name:14s} {leg:36s} " + " ".join(f"wall {r[leg][0]:8.3f} returned {r[leg][1]:8.3f}" for r in res))
        if not a.parent_root:
            say("  (no --parent-root given: the parent commit was not measured)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
