"""GPU tool: the MHST train step (forward, weighted CE over the probability mixture, backward, fused AdamW) of the
registry's model at B = 64, dropout 0.1, 16 classes, at 144 + 1 and at 30 + 1 bands: `TrainStepper.step` eager
(`use_graph=False`) and captured (`capture_step=True`: one hipGraph replay per step, fresh masks and gate noise from the
device-side seed), the kernel launches per step and the five largest kernels of the eager step with their share of the
device time (torch.profiler, a separate pass); then the 3x3x3 convolution's three MFMA kernels, the direct form of its
forward and the pyramidal convolution forward alone (HIP events) with their fraction of the fp32 MFMA peak (157.3
TFLOP/s).  DESIGN.md section 28 records the output.
usage: python tools/mhst_step.py [K] [--no-profile]"""
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vit-cnn_amd"))
import torch  # noqa: E402

PEAK_FP32_MFMA = 157.3e12
B, NCLS = 64, 16


def batch(dev, l1):
    g = torch.Generator().manual_seed(7)
    x1 = torch.rand(B, l1, 8, 8, generator=g).to(dev)
    x2 = torch.rand(B, 1, 8, 8, generator=g).to(dev)
    t = torch.randint(1, NCLS, (B,), generator=g).to(dev)
    return x1, x2, t


def timed(fn, k, dev):
    """median / min / max of k calls in ms, each between two HIP events on the current stream"""
    ts = []
    for _ in range(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def build(dev, l1):
    from vitcnn_amd import model_utils as mu
    torch.manual_seed(0)
    m, opt, crit, _ = mu.get_model("MHST", n_classes=NCLS, n_bands=(l1, 1), ignored_labels=[0], dataset="synthetic",
                                   device=dev)
    return m.train(), opt, crit


def run(l1, k, profile):
    from vitcnn_amd import seeds
    from vitcnn_amd.step import TrainStepper
    dev = torch.device("cuda", 0)
    x1, x2, t = batch(dev, l1)
    for use_graph in (False, True):
        m, opt, crit = build(dev, l1)
        seeds.attach(m, 12345)
        st = TrainStepper(m, opt, crit, capture_step=True, use_graph=use_graph)
        for _ in range(4):
            st.step(x1, x2, t)
        med, lo, hi = timed(lambda: st.step(x1, x2, t), k, dev)
        print(f"mhst {l1}+1 bands B={B} {st.launch}: median {med:.3f} ms/step (min {lo:.3f}, max {hi:.3f}) over {k} steps",
              flush=True)
        if profile and not use_graph:
            from torch.profiler import ProfilerActivity, profile as prof
            try:
                with prof(activities=[ProfilerActivity.CUDA]) as p:
                    for _ in range(3):
                        st.step(x1, x2, t)
                    torch.cuda.synchronize(dev)
                evs = [e for e in p.key_averages() if getattr(e, "device_time_total", 0) > 0]
                total = sum(e.device_time_total for e in evs)
                evs.sort(key=lambda e: -e.device_time_total)
                for e in evs[:5]:
                    print(f"  kernel {e.key[:90]}: {e.device_time_total / 3e3:.3f} ms/step, "
                          f"{100.0 * e.device_time_total / total:.1f}% of the device time ({e.count // 3} launches)")
                print(f"  device time {total / 3e3:.3f} ms/step, {sum(e.count for e in evs) / 3:.0f} launches/step",
                      flush=True)
            except Exception as e:   # the profiler is optional: say so, never guess
                print(f"  kernel shares not measured: {type(e).__name__}: {str(e)[:120]}", flush=True)


def conv_alone(l1, k):
    """the 3x3x3 conv and the HSI pyramidal conv (four launches) forward, alone: time and fraction of the MFMA peak"""
    from vitcnn_amd._lib import lib
    L = lib()
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    D1 = (l1 + 2) // 3
    x = torch.rand(B * D1 * 64, 16, device=dev)
    w3, b3, y3 = torch.rand(16 * 16 * 27, device=dev), torch.rand(16, device=dev), torch.empty(B * D1 * 64, 16, device=dev)

    n3 = L.vc_mhst_conv3_wgrad_ws_floats(B, D1)
    ws3, dw3 = torch.empty(n3, device=dev), torch.empty(16 * 16 * 27, device=dev)

    def c3():
        L.vc_mhst_conv3_fwd(B, D1, x.data_ptr(), 16, w3.data_ptr(), b3.data_ptr(), y3.data_ptr(), 16, s)

    def c3d():
        L.vc_mhst_conv3_dgrad(B, D1, x.data_ptr(), 16, w3.data_ptr(), y3.data_ptr(), 16, 0.0, s)

    def c3w():
        L.vc_mhst_conv3_wgrad(B, D1, x.data_ptr(), 16, y3.data_ptr(), 16, dw3.data_ptr(), ws3.data_ptr(), n3, s)

    def c3direct():
        L.vc_mhst_conv_fwd(B, D1, 8, 8, 16, 16, 1, 3, 3, 1, 1, D1, x.data_ptr(), 16, w3.data_ptr(), b3.data_ptr(),
                           y3.data_ptr(), 16, s)

    ws = [torch.rand(16 * (16 // g) * D1 * kk * kk, device=dev) for kk, g in zip((3, 5, 7, 9), (1, 2, 4, 8))]
    y4 = torch.empty(B * 64, 64, device=dev)

    def py():
        for i, (kk, g) in enumerate(zip((3, 5, 7, 9), (1, 2, 4, 8))):
            L.vc_mhst_conv_fwd(B, D1, 8, 8, 16, 16, g, D1, kk, 1, 0, 1, x.data_ptr(), 16, ws[i].data_ptr(), None,
                               y4.data_ptr() + 64 * i, 64, s)

    f3 = 2.0 * B * D1 * 64 * 16 * 432
    fp = 2.0 * B * 64 * 16 * sum((16 // g) * D1 * kk * kk for kk, g in zip((3, 5, 7, 9), (1, 2, 4, 8)))
    for name, fn, fl in (("3x3x3 conv fwd (MFMA)", c3, f3), ("3x3x3 conv dgrad (MFMA)", c3d, f3),
                         ("3x3x3 conv wgrad (MFMA, 2 launches)", c3w, f3), ("3x3x3 conv fwd (direct form)", c3direct, f3),
                         ("pyramidal conv fwd (4 launches)", py, fp)):
        for _ in range(5):
            fn()
        med, lo, hi = timed(fn, k, dev)
        print(f"  {l1} bands {name}: median {med:.3f} ms (min {lo:.3f}), {fl / 1e6 / B:.1f} MFLOP/patch nominal, "
              f"{100.0 * fl / (lo * 1e-3) / PEAK_FP32_MFMA:.2f}% of the fp32 MFMA peak at the minimum", flush=True)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    k = int(args[0]) if args else 30
    for l1 in (144, 30):
        run(l1, k, "--no-profile" not in sys.argv)
        conv_alone(l1, k)


if __name__ == "__main__":
    main()
