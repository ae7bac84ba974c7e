"""GPU tool: the GLT-Net train step (forward, GLT_Loss = weighted CE + reconstruction loss, backward, fused Adam) of the
registry's model at B = 64, dropout 0.1, 16 classes, 24 x 24 windows (P = 8), at 144 + 1 and at 30 + 1 bands:
`TrainStepper.step` eager (`use_graph=False`) and captured (`capture_step=True`: one hipGraph replay per step, fresh
masks from the device-side seed), the kernel launches per step and the largest kernels of the eager step with their
share of the device time (torch.profiler, a separate pass); then the decoder's up-conv kernels alone (HIP events) with
their fraction of the fp32 MFMA peak (157.3 TFLOP/s; the FLOPs are the nominal 2 * 9 * C * O per output pixel of the
upsampled map), A/B against the same convolution composed from the existing entry points on a materialised upsampled
tensor (torch's repeat_interleave, then vc_conv3x3_tap_*; the data gradient's s x s replica sum by a torch reduction),
the two alternating sample by sample.  DESIGN.md section 29 records the output.
usage: python tools/glt_step.py [K] [--no-profile]"""
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vit-cnn_amd"))
import torch  # noqa: E402

PEAK_FP32_MFMA = 157.3e12
B, NCLS, P = 64, 16, 8


def batch(dev, l1):
    g = torch.Generator().manual_seed(7)
    x1 = torch.rand(B, l1, 3 * P, 3 * P, generator=g).to(dev)
    x2 = torch.rand(B, 1, 3 * P, 3 * P, generator=g).to(dev)
    t = torch.randint(1, NCLS, (B,), generator=g).to(dev)
    return x1, x2, t


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(fn, k):
    """median / min / max of k calls in ms, each between two HIP events on the current stream"""
    ts = [once(fn) for _ in range(k)]
    return statistics.median(ts), min(ts), max(ts)


def build(dev, l1):
    from vitcnn_amd import model_utils as mu
    torch.manual_seed(0)
    m, opt, crit, _ = mu.get_model("GLT_Net", n_classes=NCLS, n_bands=(l1, 1), ignored_labels=[0], dataset="synthetic",
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
        med, lo, hi = timed(lambda: st.step(x1, x2, t), k)
        print(f"glt {l1}+1 bands B={B} {st.launch}: median {med:.3f} ms/step (min {lo:.3f}, max {hi:.3f}) over {k} steps",
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
                for e in evs[:8]:
                    print(f"  kernel {e.key[:90]}: {e.device_time_total / 3e3:.3f} ms/step, "
                          f"{100.0 * e.device_time_total / total:.1f}% of the device time ({e.count // 3} launches)")
                print(f"  device time {total / 3e3:.3f} ms/step, {sum(e.count for e in evs) / 3:.0f} launches/step",
                      flush=True)
            except Exception as e:   # the profiler is optional: say so, never guess
                print(f"  kernel shares not measured: {type(e).__name__}: {str(e)[:120]}", flush=True)


def upconv_alone(O, k):
    """the three up-conv kernels at C = 64 -> O, s in {1, 2, 3}, alone, against materialise + the existing conv"""
    from vitcnn_amd._lib import lib
    L = lib()
    dev = torch.device("cuda", 0)
    s_ = torch.cuda.current_stream(dev).cuda_stream
    C, ld = 64, (O + 3) // 4 * 4
    ws = torch.empty(1 << 22, device=dev)
    x = torch.rand(B * P * P, C, device=dev)
    w, bias = torch.rand(O, C, 3, 3, device=dev) - 0.5, torch.rand(O, device=dev)
    wt = torch.empty(O * 9 * C, device=dev)
    L.vc_conv3x3_pack(O, C, 0, w.data_ptr(), wt.data_ptr(), 0.0, s_)
    dw, db, dx = torch.empty_like(w), torch.empty_like(bias), torch.empty_like(x)
    for sc in (1, 2, 3):
        S = sc * P
        y = torch.empty(B * S * S, ld, device=dev)
        dy = torch.rand(B * S * S, ld, device=dev)
        up = torch.empty(B * S * S, C, device=dev)
        dup = torch.empty(B * S * S, C, device=dev)
        wsp, wsn = ws.data_ptr(), ws.numel()

        def materialise():
            up.copy_(x.view(B, P, P, C).repeat_interleave(sc, 1).repeat_interleave(sc, 2).reshape(B * S * S, C))

        def f_new():
            L.vc_glt_upconv_fwd(B, P, sc, C, O, x.data_ptr(), C, wt.data_ptr(), bias.data_ptr(), y.data_ptr(), ld, wsp,
                                wsn, s_)

        def f_old():
            materialise()
            L.vc_conv3x3_tap_fwd(B, S, S, C, O, 1, up.data_ptr(), C, wt.data_ptr(), bias.data_ptr(), y.data_ptr(), ld,
                                 wsp, wsn, s_)

        def w_new():
            L.vc_glt_upconv_wgrad(B, P, sc, C, O, x.data_ptr(), C, dy.data_ptr(), ld, dw.data_ptr(), db.data_ptr(), wsp,
                                  wsn, s_)

        def w_old():      # the forward's materialised tensor would be kept: not charged again
            L.vc_conv3x3_tap_wgrad_oihw(B, S, S, C, O, 1, up.data_ptr(), C, dy.data_ptr(), ld, dw.data_ptr(),
                                        db.data_ptr(), wsp, wsn, s_)

        def d_new():
            L.vc_glt_upconv_dgrad(B, P, sc, C, O, dy.data_ptr(), ld, wt.data_ptr(), 0.0, dx.data_ptr(), C, wsp, wsn, s_)

        def d_old():
            L.vc_conv3x3_tap_dgrad(B, S, S, C, O, 1, dy.data_ptr(), ld, wt.data_ptr(), 0.0, dup.data_ptr(), C, wsp, wsn,
                                   s_)
            dx.copy_(dup.view(B, P, sc, P, sc, C).sum((2, 4)).reshape(B * P * P, C))

        flops = 2.0 * B * S * S * 9 * C * O
        for name, new, old in (("fwd", f_new, f_old), ("wgrad", w_new, w_old), ("dgrad", d_new, d_old)):
            for _ in range(5):
                new()
                old()
            tn, to = [], []
            for _ in range(k):      # interleaved samples
                tn.append(once(new))
                to.append(once(old))
            print(f"  upconv {name} 64 -> {O}, s = {sc}: fused median {statistics.median(tn):.4f} ms (min {min(tn):.4f}), "
                  f"{100.0 * flops / (min(tn) * 1e-3) / PEAK_FP32_MFMA:.2f}% of the fp32 MFMA peak at the minimum "
                  f"({flops / 1e6 / B:.1f} MFLOP/patch nominal); materialise + existing conv median "
                  f"{statistics.median(to):.4f} ms (min {min(to):.4f})", flush=True)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    k = int(args[0]) if args else 30
    for l1 in (144, 30):
        run(l1, k, "--no-profile" not in sys.argv)
        upconv_alone(l1, k)
    upconv_alone(1, k)


if __name__ == "__main__":
    main()
