"""GPU tool: the HCTnet train step (forward, weighted CE, backward, fused Adam) at B = 64, patch 11, 16 classes,
6 tokens, dropout 0.1: the eager step's median time after warm-up, the same step captured as one hipGraph and
replayed (if capture works), the kernel launches per step and the largest kernels of the eager step with their share
of the device time (torch.profiler, a separate pass).  DESIGN.md section 22 records the output.
usage: python tools/hct_step.py [K] [--no-profile]
       python tools/hct_step.py --cpu-reference TREE    (no GPU: the reference module of TREE in fp32 on 8 CPU threads,
                                                         forward + CE + backward + torch.optim.Adam, median of 5 after 3)"""
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vit-cnn_amd"))
import torch  # noqa: E402


def batch(dev):
    g = torch.Generator().manual_seed(7)
    x1 = torch.rand(64, 3, 11, 11, generator=g).to(dev)
    x2 = torch.rand(64, 1, 11, 11, generator=g).to(dev)
    t = torch.randint(1, 16, (64,), generator=g).to(dev)
    w = torch.ones(16, device=dev)
    w[0] = 0.0
    return x1, x2, t, w


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


def run(k, profile):
    from vitcnn_amd import AdamW, CrossEntropyLoss
    from vitcnn_amd.hctnet import HCTnet
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = HCTnet(num_classes=16, num_tokens=6, heads=8).to(dev).train()
    opt = AdamW(m.parameters(), lr=1e-4, weight_decay=0.0)
    x1, x2, t, w = batch(dev)
    crit = CrossEntropyLoss(weight=w)

    def step():
        opt.zero_grad(set_to_none=True)
        crit(m(x1, x2), t).backward()
        opt.step()

    for _ in range(5):
        step()
    med, lo, hi = timed(step, k, dev)
    print(f"hctnet B=64 eager: median {med:.3f} ms/step (min {lo:.3f}, max {hi:.3f}) over {k} steps", flush=True)
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
            print(f"  device time {total / 5e3:.3f} ms/step, {sum(e.count for e in evs) / 5:.0f} launches/step", flush=True)
        except Exception as e:   # the profiler is optional: say so, never guess
            print(f"  kernel shares not measured: {type(e).__name__}: {str(e)[:120]}", flush=True)
    # the same step as one hipGraph (the keep masks' seed is drawn on the host at capture: every replay repeats it)
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
        print(f"hctnet B=64 hipGraph: median {med:.3f} ms/step (min {lo:.3f}, max {hi:.3f}) over {k} replays", flush=True)
    except Exception as e:
        torch.cuda.synchronize(dev)
        print(f"hctnet hipGraph: capture failed ({type(e).__name__}: {str(e)[:120]}); not measured", flush=True)


def cpu_reference(tree):
    import importlib.util
    import types
    for name in ("torchvision", "torchsummary"):   # imported by the reference file, never used
        if name not in sys.modules:
            stub = types.ModuleType(name)
            stub.summary = None
            sys.modules[name] = stub
    spec = importlib.util.spec_from_file_location("ref_hctnet", os.path.join(tree, "model", "compare_method", "HCTnet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.set_num_threads(8)
    torch.manual_seed(0)
    net = mod.HCTnet(num_classes=16, num_tokens=6, heads=8).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    x1, x2, t, w = batch("cpu")
    ts = []
    for i in range(8):
        t0 = time.perf_counter()
        opt.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(net(x1, x2), t, weight=w).backward()
        opt.step()
        if i >= 3:
            ts.append((time.perf_counter() - t0) * 1e3)
    print(f"hctnet B=64 reference module, fp32, 8 CPU threads: median {statistics.median(ts):.2f} ms/step "
          f"(min {min(ts):.2f}, max {max(ts):.2f}) over 5 steps after 3")


def main():
    if "--cpu-reference" in sys.argv:
        return cpu_reference(sys.argv[sys.argv.index("--cpu-reference") + 1])
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    k = int(args[0]) if args else 300
    run(k, "--no-profile" not in sys.argv)


if __name__ == "__main__":
    main()
