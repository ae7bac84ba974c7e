#!/usr/bin/env python3
"""A/B of the captured ViT-CNN training step at two band counts, possibly on two builds of the package.

    python tools/bands_step_bench.py --a .:63 --b path/to/other/checkout:64 --out profiles/bands63_step.json

Each side `ROOT:BANDS` is a checkout root (holding vit-cnn_amd/ with its built library) and an HSI band count.  A
worker process per side builds the model (B = 64, P = 9, 1 LiDAR band, 16 classes, hash-filled parameters, a
synthetic batch), runs the fused training step (forward, CE, backward, AdamW) eagerly three times, captures it into
one hipGraph and waits.  The coordinator then alternates the two workers: per repetition each replays the graph
`--warm` times untimed and `--steps` times between two device events.  Per side: every repetition's ms / step, the
median and the spread (max - min).  The pass condition printed and stored: median(a) - median(b) <= 2 x spread(b).
Both workers hold the GPU open for the whole run; only one replays at a time."""
import argparse
import json
import os
import statistics
import subprocess
import sys


def worker(root, bands, batch, patch, replays=0):
    sys.path[:0] = [os.path.join(root, "vit-cnn_amd")]
    import torch
    from vitcnn_amd import AdamW, CrossEntropyLoss, Multimodality_Mamba, fused_train_step
    from vitcnn_amd.hashinit import fill_module_, synthetic_batch
    dev = torch.device("cuda:0")
    m = Multimodality_Mamba(patch, 1, 1, bands, 1, 32, 16, "multi_clock_gate")
    fill_module_(m)
    m = m.to(dev).train()
    hsi, lidar, tgt = (torch.from_numpy(a).to(dev) for a in synthetic_batch("bands.bench", batch, bands, 1, patch, 16))
    w = torch.ones(16)
    w[0] = 0.0
    crit = CrossEntropyLoss(weight=w.to(dev))
    opt = AdamW(m.parameters(), lr=8e-4)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            fused_train_step(m, crit, hsi, lidar, tgt, optimizer=opt)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    opt.sync_hyper()
    opt.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    holder = {}
    with torch.cuda.graph(graph):
        holder["loss"] = fused_train_step(m, crit, hsi, lidar, tgt, optimizer=opt)
    torch.cuda.synchronize()
    if replays:   # a fixed number of replays and out: the process a profiler wraps
        for _ in range(replays):
            graph.replay()
        torch.cuda.synchronize()
        return
    print("ready", flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        warm, steps = int(cmd[1]), int(cmd[2])
        for _ in range(warm):
            graph.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        print("ms %.6f %.6f" % (e0.elapsed_time(e1) / steps, float(holder["loss"])), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", default=".:63")
    ap.add_argument("--b", default=".:64")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--patch", type=int, default=9)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=100)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", nargs=2, metavar=("ROOT", "BANDS"))
    ap.add_argument("--replays", type=int, default=0, help="with --worker: replay this often and exit (for "
                    "rocprofv3 --kernel-trace --stats -- python tools/bands_step_bench.py --worker . 63 --replays 50)")
    a = ap.parse_args()
    if a.worker:
        return worker(os.path.abspath(a.worker[0]), int(a.worker[1]), a.batch, a.patch, a.replays)
    sides, procs = {}, {}
    try:
        for key in ("a", "b"):
            root, bands = getattr(a, key).rsplit(":", 1)
            sides[key] = dict(root=root, bands=int(bands), ms=[])
            procs[key] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root, bands, "--batch",
                                           str(a.batch), "--patch", str(a.patch)], stdin=subprocess.PIPE,
                                          stdout=subprocess.PIPE, text=True)
            if procs[key].stdout.readline().strip() != "ready":
                raise RuntimeError(f"worker {key} did not come up (exit {procs[key].poll()})")
        for _ in range(a.reps):
            for key in ("a", "b"):
                p = procs[key]
                p.stdin.write(f"go {a.warm} {a.steps}\n")
                p.stdin.flush()
                ans = p.stdout.readline().split()
                if len(ans) != 3 or ans[0] != "ms":
                    raise RuntimeError(f"worker {key} failed (exit {p.poll()}): {ans}")
                sides[key]["ms"].append(float(ans[1]))
    finally:
        for p in procs.values():
            try:
                if p.poll() is None:
                    p.stdin.write("quit\n")
                    p.stdin.flush()
                p.wait(timeout=60)
            except Exception:
                p.kill()
    for s in sides.values():
        s["median_ms"] = statistics.median(s["ms"])
        s["spread_ms"] = max(s["ms"]) - min(s["ms"])
    diff = sides["a"]["median_ms"] - sides["b"]["median_ms"]
    res = dict(what="captured training step (forward, CE, backward, fused AdamW), ms per graph replay",
               batch=a.batch, patch=a.patch, reps=a.reps, warm=a.warm, steps=a.steps, a=sides["a"], b=sides["b"],
               a_minus_b_ms=diff, bound_ms=2.0 * sides["b"]["spread_ms"],
               a_not_slower_than_b=bool(diff <= 2.0 * sides["b"]["spread_ms"]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
