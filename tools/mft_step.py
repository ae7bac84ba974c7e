"""GPU tool: the MFT train step (forward, weighted CE, backward, fused Adam with coupled L2) at B = 64, patch 11, with
30 bands and with 144 bands: the eager step's median time after warm-up, the same step captured as one hipGraph
and replayed (if capture works), and the largest kernels of the eager step with their share of the device time
(torch.profiler, a separate pass).  DESIGN.md section 16 records the output.
usage: python tools/mft_step.py [K] [--no-profile]"""
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vit-cnn_amd"))
import torch  # noqa: E402

from vitcnn_amd import CrossEntropyLoss  # noqa: E402
from vitcnn_amd.mft import MFT  # noqa: E402
from vitcnn_amd.optim import Adam  # noqa: E402


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


def run(nc, k, profile):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = MFT(patch_size=11, FM=16, NC=nc, NCLidar=1, Classes=16, HSIOnly=False).to(dev).train()
    opt = Adam(m.parameters(), lr=5e-4, weight_decay=5e-3)
    w = torch.ones(16, device=dev)
    w[0] = 0.0
    crit = CrossEntropyLoss(weight=w)
    g = torch.Generator().manual_seed(7)
    x1 = torch.rand(64, nc, 11, 11, generator=g).to(dev)
    x2 = torch.rand(64, 1, 11, 11, generator=g).to(dev)
    t = torch.randint(1, 16, (64,), generator=g).to(dev)

    def step():
        opt.zero_grad(set_to_none=True)
        crit(m(x1, x2), t).backward()
        opt.step()

    for _ in range(5):
        step()
    med, lo, hi = timed(step, k, dev)
    print(f"mft NC={nc} B=64 eager: median {med:.3f} ms/step (min {lo:.3f}, max {hi:.3f}) over {k} steps", flush=True)
    if profile:
        from torch.profiler import ProfilerActivity, profile as prof
        try:
            with prof(activities=[ProfilerActivity.CUDA]) as p:
                for _ in range(5):
                    step()
                torch.cuda.synchronize(dev)
            evs = [e for e in p.key_averages() if getattr(e, "device_time_total", 0) > 0]
            total = sum(e.device_time_total for e in evs)
            evs.sort(key=lambda e: -e.device_time_total)
            for e in evs[:6]:
                print(f"  kernel {e.key[:90]}: {e.device_time_total / 5e3:.3f} ms/step, "
                      f"{100.0 * e.device_time_total / total:.1f}% of the device time ({e.count // 5} launches)")
            print(f"  device time {total / 5e3:.3f} ms/step", flush=True)
        except Exception as e:   # the profiler is optional: say so, never guess
            print(f"  kernel shares not measured: {type(e).__name__}: {str(e)[:120]}", flush=True)
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
        print(f"mft NC={nc} B=64 hipGraph: median {med:.3f} ms/step (min {lo:.3f}, max {hi:.3f}) over {k} replays",
              flush=True)
    except Exception as e:
        torch.cuda.synchronize(dev)
        print(f"mft NC={nc} hipGraph: capture failed ({type(e).__name__}: {str(e)[:120]}); not measured", flush=True)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    k = int(args[0]) if args else 50
    for nc in (30, 144):
        run(nc, k, "--no-profile" not in sys.argv)


if __name__ == "__main__":
    main()
