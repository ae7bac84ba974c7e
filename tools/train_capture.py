"""GPU tool: `TrainStepper.step` of the comparison models with `capture_step` False (the eager sequence) and True (one
hipGraph replay per batch, the dropout seed advanced on the device) at B = 64 with dropout 0.1: HCTnet (patch 11, 16
classes, 6 tokens), MFT (30 bands, patch 11), SpectralFormer (144 + 1 bands) and S2EFT (144 + 1 bands, patch 7, over
the two patches).  Per model and mode: the median step
time of 300 steps after 5 (each ended by a device synchronise, host clock, as tools/hct_step.py) and the kernel launches
per step (torch.profiler, a separate pass of 5 steps).  DESIGN.md section 23 records the output.
usage: python tools/train_capture.py [MODEL ...] [K]     MODEL: hctnet | mft | spectralformer | s2eft (default: all), K steps (300)"""
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vit-cnn_amd"))
import torch  # noqa: E402

P_DROP = 0.1


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


def build(tag, dev):
    """(model, optimizer, criterion, batch) as get_model / the per-model step tools build them"""
    from vitcnn_amd import CrossEntropyLoss
    from vitcnn_amd import model_utils as mu
    from vitcnn_amd.optim import Adam, AdamW
    g = torch.Generator().manual_seed(7)
    w = torch.ones(16, device=dev)
    w[0] = 0.0
    crit = CrossEntropyLoss(weight=w)
    if tag == "hctnet":
        from vitcnn_amd.hctnet import HCTnet
        m = HCTnet(num_classes=16, num_tokens=6, heads=8).to(dev)
        opt = AdamW(m.parameters(), lr=1e-4, weight_decay=0.0)
        shapes = ((3, 11, 11), (1, 11, 11))
    elif tag == "mft":
        from vitcnn_amd.mft import MFT
        m = MFT(patch_size=11, FM=16, NC=30, NCLidar=1, Classes=16, HSIOnly=False).to(dev)
        opt = Adam(m.parameters(), lr=5e-4, weight_decay=5e-3)
        shapes = ((30, 11, 11), (1, 11, 11))
    elif tag == "s2eft":
        m, opt, crit, _ = mu.get_model("S2EFT", n_classes=16, n_bands=(144, 1), ignored_labels=[0],
                                       dataset="Houston2013", device=dev)
        shapes = ((144, 7, 7), (1, 7, 7))
    else:
        m, opt, crit, _ = mu.get_model("SpectralFormer", n_classes=16, n_bands=(144, 1), ignored_labels=[0],
                                       dataset="Houston2013", device=dev)
        shapes = ((144, 1, 1), (1, 1, 1))
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = P_DROP
    x1 = torch.rand(64, *shapes[0], generator=g).to(dev)
    x2 = torch.rand(64, *shapes[1], generator=g).to(dev)
    t = torch.randint(1, 16, (64,), generator=g).to(dev)
    return m.train(), opt, crit, (x1, x2, t)


def launches(fn, dev):
    from torch.profiler import ProfilerActivity, profile as prof
    try:
        with prof(activities=[ProfilerActivity.CUDA]) as p:
            for _ in range(5):
                fn()
            torch.cuda.synchronize(dev)
        evs = [e for e in p.key_averages() if getattr(e, "device_time_total", 0) > 0]
        return f"{sum(e.count for e in evs) / 5:.0f} launches/step, device time {sum(e.device_time_total for e in evs) / 5e3:.3f} ms/step"
    except Exception as e:   # the profiler is optional: say so, never guess
        return f"launches not measured ({type(e).__name__}: {str(e)[:100]})"


def run(tag, k):
    from vitcnn_amd import seeds
    from vitcnn_amd.step import TrainStepper
    dev = torch.device("cuda", 0)
    for capture in (False, True):
        torch.manual_seed(0)
        m, opt, crit, (x1, x2, t) = build(tag, dev)
        stepper = TrainStepper(m, opt, crit, capture_step=capture)

        def step():
            stepper.step(x1, x2, t)

        for _ in range(5):
            step()
        med, lo, hi = timed(step, k, dev)
        st = seeds.state(m)
        print(f"{tag} B=64 dropout {P_DROP} (masks drawn: {seeds.has_dropout(m)}) capture_step={capture}: launch "
              f"'{stepper.launch}', median {med:.3f} ms/step (min {lo:.3f}, max {hi:.3f}) over {k} steps; "
              f"{launches(step, dev)}; device seed step {st.read()[1] if st is not None else 'none'}", flush=True)


def main():
    args = sys.argv[1:]
    k = int(args.pop()) if args and args[-1].isdigit() else 300
    for tag in args or ["hctnet", "mft", "spectralformer", "s2eft"]:
        if tag not in ("hctnet", "mft", "spectralformer", "s2eft"):
            raise SystemExit(f"unknown model {tag}")
        run(tag, k)


if __name__ == "__main__":
    main()
