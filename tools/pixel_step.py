"""GPU tool: the train step (forward, criterion, backward, fused Adam) of the per-pixel models EndNet and SpectralFormer
at B = 64 on the Houston2013 shape (144 + 1 bands, patch 1, 16 classes), as get_model builds them: the number of
kernel launches of one step and their device time (torch.profiler), the eager step's median time after warm-up, and
the same step captured as one hipGraph and replayed (if capture works), all on a single stream.  DESIGN.md section 21
records the output; nothing here is gated.
usage: python tools/pixel_step.py [MODEL ...] [K]     MODEL: endnet | spectralformer (default: both), K steps (50)"""
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vit-cnn_amd"))
import torch  # noqa: E402

from vitcnn_amd import model_utils as mu  # noqa: E402

NAMES = {"endnet": "EndNet", "spectralformer": "SpectralFormer"}


def timed(fn, k, dev):
    """median / min / max of k calls, each ended by a device synchronise (host clock)"""
    ts = []
    for _ in range(k):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def run(tag, k):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m, opt, crit, _ = mu.get_model(NAMES[tag], n_classes=16, n_bands=(144, 1), ignored_labels=[0],
                                   dataset="Houston2013", device=dev)
    m.train()
    g = torch.Generator().manual_seed(7)
    x1 = torch.rand(64, 144, 1, 1, generator=g).to(dev)      # what PatchBatcher yields at patch_size 1
    x2 = torch.rand(64, 1, 1, 1, generator=g).to(dev)
    t = torch.randint(1, 16, (64,), generator=g).to(dev)

    def step():
        opt.zero_grad(set_to_none=True)
        crit(m(x1, x2), t).backward()
        opt.step()

    for _ in range(5):
        step()
    torch.cuda.synchronize(dev)
    from torch.profiler import ProfilerActivity, profile as prof
    try:
        with prof(activities=[ProfilerActivity.CUDA]) as p:
            step()
            torch.cuda.synchronize(dev)
        evs = [e for e in p.key_averages() if getattr(e, "device_time_total", 0) > 0]
        launches = sum(e.count for e in evs)
        total = sum(e.device_time_total for e in evs)
        print(f"{tag} B=64: {launches} device launches per step, device time {total / 1e3:.3f} ms", flush=True)
        evs.sort(key=lambda e: -e.device_time_total)
        for e in evs[:6]:
            print(f"  kernel {e.key[:90]}: {e.device_time_total / 1e3:.3f} ms ({e.count} launches)")
    except Exception as e:   # the profiler is optional: say so, never guess
        print(f"{tag}: launch count not measured: {type(e).__name__}: {str(e)[:120]}", flush=True)
    med, lo, hi = timed(step, k, dev)
    print(f"{tag} B=64 eager: median {med:.3f} ms/step (min {lo:.3f}, max {hi:.3f}) over {k} steps", flush=True)
    # the same step as one hipGraph
    try:
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        opt.zero_grad(set_to_none=True)
        opt.sync_hyper()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            crit(m(x1, x2), t).backward()
            opt.step()
        for _ in range(5):
            graph.replay()
        med, lo, hi = timed(graph.replay, k, dev)
        print(f"{tag} B=64 hipGraph: median {med:.3f} ms/step (min {lo:.3f}, max {hi:.3f}) over {k} replays",
              flush=True)
    except Exception as e:
        torch.cuda.synchronize(dev)
        print(f"{tag} hipGraph: capture failed ({type(e).__name__}: {str(e)[:120]}); not measured", flush=True)


def main():
    args = sys.argv[1:]
    k = next((int(a) for a in args if a.isdigit()), 50)
    tags = [a for a in args if a in NAMES] or list(NAMES)
    for tag in tags:
        run(tag, k)


if __name__ == "__main__":
    main()
