#!/usr/bin/env python3
"""Training from a list of device rollout buffers, on one MI355X -> profiles/buffer_list_bench.txt ("A list of buffers";
INTEGRATION.md §5b, §5m).

K = 3 buffers per shape, the shapes of tools/diag/epoch_bench.py: "wide" = 4096 envs x 64 steps, chunks of 8; "reference" = 32 envs x
3000 steps, chunks of 60; 5 minibatches, 4 epochs. Per shape:

(a) one ``DeviceReplayBuffer.epoch_of([b0, b1, b2], ...)`` (three ``queue_advantages`` and ONE gather launch) against what could be done
    before it: three ``epoch()`` calls, one per buffer, each with minibatches of a third the size, and per minibatch and field one
    ``torch.cat`` of the three parts along the chunk axis (so that the rows come out step-major, as the update reads them). The two do not
    draw the same minibatches (the second never puts a chunk across two buffers and takes a third of every minibatch from each); they
    move the same number of floats. Wall time: a host clock around the call and one synchronise, the legs alternating call by call.
(b) a whole ``DevicePPOTrainer.train`` on the list, the tests' restated policy with the three swaps: the default path (the generator)
    against ``stream_ordered=True`` (``epoch_of``).
(c) the single-buffer paths this change leaves alone, ``buffer.epoch`` and the default ``train`` on one buffer, with this tree's library
    and, with ``--parent-root``, with a checkout of the parent commit built in that directory. Each tree is measured in two processes,
    the trees alternating; the margin is the parent's own spread from run to run and from process to process.

Every measurement is a child process of its own under a time limit; the first one that fails ends the run. ``--runs`` consecutive runs
are on the page so that the spread is.

    python tools/diag/buffer_list_bench.py [--runs 3] [--reps 10] [--shapes wide,reference] [--parent-root DIR]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import epoch_bench as EB  # noqa: E402  (the shapes, the buffers' contents, the restated policy and the alternating timer)

ROOT = EB.ROOT
K = 3


def list_orders(s, n):
    import numpy as np
    return [np.random.default_rng(e).permutation(s["E"] * (s["T"] * K) // s["L"]) for e in range(n)]


def child_gather(a):
    torch, pkg = EB.child_setup(a.root)
    s = EB.SHAPES[a.shape]
    n_mb, L = s["n_mb"], s["L"]
    bufs = [EB.make_buffer(torch, pkg, s, False, seed=1 + k) for k in range(K)]
    order, single = list_orders(s, 1)[0], EB.orders_for(s, 1)[0]
    hid = (bufs[0].recurrent_hidden_layers, bufs[0].recurrent_hidden_size)

    def listed():
        return pkg.DeviceReplayBuffer.epoch_of(bufs, n_mb, L, chunk_order=order)

    def one_by_one():
        eps = [b.epoch(n_mb, L, chunk_order=single) for b in bufs]
        out = []
        for i in range(n_mb):
            item = []
            for f, name in enumerate(eps[0].names):
                parts = [e[i][f] for e in eps]
                if name.startswith("rnn_states"):
                    item.append(torch.cat(parts, 0))
                else:
                    item.append(torch.cat([p.view(L, -1, p.shape[-1]) for p in parts], 1).view(-1, parts[0].shape[-1]))
            out.append(tuple(item))
        return out

    a_, b_ = listed(), one_by_one()
    torch.cuda.synchronize()
    # the same fields of (but for the remainders of the two divisions) the same size
    assert all(x.shape[1:] == y.shape[1:] and 0 <= x.shape[0] - y.shape[0] < K * L for x, y in zip(a_[0], b_[0])) and a_[0][-1].shape[1:] == hid
    del a_, b_
    legs = {"epoch_of": listed, "3 x epoch + cat": one_by_one}
    print("RESULT " + json.dumps([EB.alternate(torch, legs, a.reps) for _ in range(a.runs)]))


def child_train(a):
    torch, pkg = EB.child_setup(a.root)
    s = EB.SHAPES[a.shape]
    bufs, tr = [EB.train_buffer(torch, pkg, s) for _ in range(K)], EB.trainer_for(torch, pkg, s)
    orders = list_orders(s, s["epochs"])
    pols = {k: EB.restated_policy(torch, pkg) for k in ("default", "stream_ordered")}
    legs = {"default": lambda: tr.train(pols["default"], bufs, chunk_orders=orders),
            "stream_ordered": lambda: tr.train(pols["stream_ordered"], bufs, chunk_orders=orders, stream_ordered=True)}
    print("RESULT " + json.dumps([EB.alternate(torch, legs, a.reps) for _ in range(a.runs)]))


def child_untouched(a):
    """(c): one buffer's epoch() and default train with the package of a.root (this tree, or a built checkout of the parent)."""
    torch, pkg = EB.child_setup(a.root)
    s = EB.SHAPES[a.shape]
    buf, tr = EB.train_buffer(torch, pkg, s), EB.trainer_for(torch, pkg, s)
    orders = EB.orders_for(s, s["epochs"])
    pol = EB.restated_policy(torch, pkg)
    legs = {"train": lambda: tr.train(pol, buf, chunk_orders=orders), "epoch": lambda: buf.epoch(s["n_mb"], s["L"], chunk_order=orders[0])}
    print("RESULT " + json.dumps([EB.alternate(torch, legs, a.reps) for _ in range(a.runs)]))


CHILDREN = {"gather": child_gather, "train": child_train, "untouched": child_untouched}


def run_child(argv, limit):
    cmd = [sys.executable, os.path.abspath(__file__)] + argv
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"buffer_list_bench: child {' '.join(argv)} ended with {p.returncode}; nothing more is started")
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise SystemExit(f"buffer_list_bench: child {' '.join(argv)} printed no result")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="wide,reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "buffer_list_bench.txt"))
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    ap.add_argument("--child", default="")
    ap.add_argument("--shape", default="wide")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return CHILDREN[a.child](a)
    lines = [f"# tools/diag/buffer_list_bench.py: {a.runs} consecutive runs, each the median of {a.reps} calls (ms); the legs of a comparison",
             "# alternate call by call. wall = host clock around the call and a synchronise; returned = until the call came back to the host.",
             f"# K = {K} buffers of each shape."]
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    if rev:
        lines.append(f"# parent commit {rev} plus the working tree of this change")

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def row(res, leg):
        return " ".join(f"wall {r[leg][0]:8.3f} returned {r[leg][1]:8.3f}" for r in res)

    common = ["--runs", str(a.runs), "--reps", str(a.reps)]
    for shape in a.shapes.split(","):
        s = EB.SHAPES[shape]
        say(f"\n== {shape}: {K} buffers of {s['E']} envs x {s['T']} steps, chunks of {s['L']}, {s['n_mb']} minibatches, {s['epochs']} epochs")
        res = run_child(["--child", "gather", "--shape", shape] + common, a.limit)
        say("(a) one epoch's minibatches from the three buffers (PPO buffer, obs 21, actions 7)")
        say(f"  {'epoch_of: 3 x advantages + 1 gather launch':52s} " + row(res, "epoch_of"))
        say(f"  {'3 x epoch (a third the minibatch) + cat per field':52s} " + row(res, "3 x epoch + cat"))
        res = run_child(["--child", "train", "--shape", shape] + common, a.limit)
        say("(b) DevicePPOTrainer.train on the list, the restated policy with the three swaps (obs 12)")
        for leg in ("default", "stream_ordered"):
            say(f"  {leg:52s} " + row(res, leg))
        say("(c) the untouched single-buffer paths: default train and one epoch() call; a process per line, the two trees alternating")
        roots = [("this tree", ROOT)] + ([("parent commit", os.path.abspath(a.parent_root))] if a.parent_root else [])
        for name, root in roots * 2:
            res = run_child(["--child", "untouched", "--shape", shape, "--root", root] + common, a.limit)
            for leg in ("train", "epoch"):
                say(f"  {name:14s} {leg:37s} " + row(res, leg))
        if not a.parent_root:
            say("  (no --parent-root given: the parent commit was not measured)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
