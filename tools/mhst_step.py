"""GPU tool: the MHST train step (forward, weighted CE over the probability mixture, backward, fused AdamW) of the
registry's model at B = 64, dropout 0.1, 16 classes, at 144 + 1 and at 30 + 1 bands: `TrainStepper.step` eager
(`use_graph=False`) and captured (`capture_step=True`: one hipGraph replay per step, fresh masks and gate noise from the
device-side seed), the kernel launches per step and the five largest kernels of the eager step with their share of the
device time (torch.profiler, a separate pass); then the 3x3x3 convolution's three MFMA kernels and the direct form of its
forward alone (HIP events), and every pyramidal site kind the MFMA family accepts (`vc_mhst_pconv_ok`) in each of the
three directions on both families, `vc_mhst_conv_*` and `vc_mhst_pconv_*`, with nominal and issued MFLOP per patch and
the fraction of the fp32 MFMA peak (157.3 TFLOP/s); then the front of the HSI encoder the same way: `hsi conv1`
(`vc_mhst_conv_*` against `vc_mhst_conv1_*`) and `hsi spectral` (the direct family's four launches together against the
one fused `vc_mhst_sconv_*` launch).  `--conv direct|mfma|mfma_all|both` chooses the model's conv mode for the step
timings; `both` times the three modes in one process, their samples interleaved (A, B, C, A, B, C, ...), as the
families' always are.  DESIGN.md section 28 records the output (profiles/mhst_pconv_step.log, and with the third mode
profiles/mhst_sconv_step.log).
usage: python tools/mhst_step.py [K] [--no-profile] [--conv direct|mfma|mfma_all|both]"""
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


def timed_ab(fns, k):
    """timed() for several callables with their samples interleaved (A, B, A, B, ...): [(median, min, max)] in ms"""
    ts = [[] for _ in fns]
    for _ in range(k):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[i].append(e0.elapsed_time(e1))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def build(dev, l1, conv="direct"):
    from vitcnn_amd import model_utils as mu
    torch.manual_seed(0)
    m, opt, crit, _ = mu.get_model("MHST", n_classes=NCLS, n_bands=(l1, 1), ignored_labels=[0], dataset="synthetic",
                                   device=dev, conv=conv)
    return m.train(), opt, crit


def run(l1, k, profile, convs):
    from vitcnn_amd import seeds
    from vitcnn_amd.step import TrainStepper
    dev = torch.device("cuda", 0)
    x1, x2, t = batch(dev, l1)
    for use_graph in (False, True):
        sts = []
        for conv in convs:
            m, opt, crit = build(dev, l1, conv)
            seeds.attach(m, 12345)
            st = TrainStepper(m, opt, crit, capture_step=True, use_graph=use_graph)
            for _ in range(4):
                st.step(x1, x2, t)
            sts.append(st)
        res = timed_ab([lambda st=st: st.step(x1, x2, t) for st in sts], k)
        for conv, st, (med, lo, hi) in zip(convs, sts, res):
            print(f"mhst {l1}+1 bands B={B} conv={conv} {st.launch}: median {med:.3f} ms/step (min {lo:.3f}, max {hi:.3f}) "
                  f"over {k} steps", flush=True)
        for conv, st in zip(convs, sts):
            if not profile or use_graph:
                continue
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
                    print(f"  conv={conv} kernel {e.key[:90]}: {e.device_time_total / 3e3:.3f} ms/step, "
                          f"{100.0 * e.device_time_total / total:.1f}% of the device time ({e.count // 3} launches)")
                print(f"  conv={conv} device time {total / 3e3:.3f} ms/step, {sum(e.count for e in evs) / 3:.0f} "
                      f"launches/step", flush=True)
            except Exception as e:   # the profiler is optional: say so, never guess
                print(f"  kernel shares not measured: {type(e).__name__}: {str(e)[:120]}", flush=True)


def conv_alone(l1, k):
    """the 3x3x3 conv alone, each direction and the direct form of its forward: time and fraction of the MFMA peak"""
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

    f3 = 2.0 * B * D1 * 64 * 16 * 432
    for name, fn, fl in (("3x3x3 conv fwd (MFMA)", c3, f3), ("3x3x3 conv dgrad (MFMA)", c3d, f3),
                         ("3x3x3 conv wgrad (MFMA, 2 launches)", c3w, f3), ("3x3x3 conv fwd (direct form)", c3direct, f3)):
        for _ in range(5):
            fn()
        med, lo, hi = timed(fn, k, dev)
        print(f"  {l1} bands {name}: median {med:.3f} ms (min {lo:.3f}), {fl / 1e6 / B:.1f} MFLOP/patch nominal, "
              f"{100.0 * fl / (lo * 1e-3) / PEAK_FP32_MFMA:.2f}% of the fp32 MFMA peak at the minimum", flush=True)


MFMA_FLOP = 2 * 16 * 16 * 4      # one v_mfma_f32_16x16x4_f32
CHUNK = 4                        # VC_MHST_PCONV_CHUNK


def issued_mflop(D, C, O, G, KS):
    """MFMA work per patch that csrc/mhst_pconv.hip issues (N padded to 16, tiles and taps wholly outside the map
    skipped), per direction, by the kernels' own loop structure"""
    cg, og, ps, KK = C // G, O // G, KS // 2, KS * KS
    inside = lambda v: 0 <= v < 8   # noqa: E731
    chunk = CHUNK if cg <= 16 else CHUNK // 2
    ksteps = sum((min(chunk, D - d0) * cg + 3) // 4 for d0 in range(0, D, chunk))
    rows = sum(1 for t in range(4) for kh in range(KS) if inside(2 * t + kh - ps) or inside(2 * t + 1 + kh - ps))
    fwd = G * ksteps * rows * KS
    NT, Kd = (D * cg + 15) // 16, (og * KK + 3) // 4 * 4
    steps = 0
    for tile in range(4):
        for i in range(Kd // 4):
            taps = {(4 * i + kq) // og for kq in range(4) if 4 * i + kq < og * KK}
            if any(inside(p // 8 + ps - tp // KS) and inside(p % 8 + ps - tp % KS)
                   for tp in taps for p in range(tile * 16, tile * 16 + 16)):
                steps += 1
    dgrad = G * NT * steps
    wsteps = sum(1 for kh in range(KS) for i in range(16) if inside(i // 2 + kh - ps)
                 for kw in range(KS) if any(inside((i & 1) * 4 + kq + kw - ps) for kq in range(4)))
    wgrad = G * NT * wsteps
    return {d: n * MFMA_FLOP / 1e6 for d, n in (("fwd", fwd), ("dgrad", dgrad), ("wgrad", wgrad))}


def pconv_sites(l1, k, fixed_sites):
    """every site kind vc_mhst_pconv_ok accepts, each direction, direct and mfma interleaved: ms, MFLOP per patch nominal
    and issued, fraction of the fp32 MFMA peak (nominal work over the minimum time)"""
    from vitcnn_amd._lib import lib
    L = lib()
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    D1 = (l1 + 2) // 3
    sites = [(f"hsi conv4 k{kk} g{g}", D1, 16, 16, g, kk, 16, 64) for kk, g in zip((3, 5, 7, 9), (1, 2, 4, 8))]
    if fixed_sites:   # these do not depend on the band count
        sites += [(f"lidar conv2 k{kk}", 1, 32, 16, 1, kk, 32, 64) for kk in (3, 5, 7, 9)]
        sites += [(f"classifier conv1 k{kk} g2", 1, 64, 16, 2, kk, 64, 32) for kk in (3, 5)]
    for name, D, C, O, G, KS, ldx, ldy in sites:
        assert L.vc_mhst_pconv_ok(D, C, O, G, KS, ldx, ldy) == 1
        x, dx = torch.rand(B * D * 64, ldx, device=dev), torch.zeros(B * D * 64, ldx, device=dev)
        w, dw = torch.rand(O * (C // G) * D * KS * KS, device=dev) - 0.5, torch.empty(O * (C // G) * D * KS * KS, device=dev)
        y, dy = torch.empty(B * 64, ldy, device=dev), torch.rand(B * 64, ldy, device=dev)
        n = L.vc_mhst_pconv_ws_floats(B, D, C, O, G, KS)
        ws = torch.empty(n, device=dev)
        d = (D, 8, 8, C, O, G, D, KS, 1, 0, 1)
        a = (D, C, O, G, KS)
        P = lambda t: t.data_ptr()   # noqa: E731
        pairs = {
            "fwd": (lambda: L.vc_mhst_conv_fwd(B, *d, P(x), ldx, P(w), None, P(y), ldy, s),
                    lambda: L.vc_mhst_pconv_fwd(B, *a, P(x), ldx, P(w), None, P(y), ldy, P(ws), n, s)),
            "dgrad": (lambda: L.vc_mhst_conv_dgrad(B, *d, P(dy), ldy, P(w), P(dx), ldx, 0.0, s),
                      lambda: L.vc_mhst_pconv_dgrad(B, *a, P(dy), ldy, P(w), P(dx), ldx, 0.0, P(ws), n, s)),
            "wgrad": (lambda: L.vc_mhst_conv_wgrad(B, *d, P(x), ldx, P(dy), ldy, P(dw), None, s),
                      lambda: L.vc_mhst_pconv_wgrad(B, *a, P(x), ldx, P(dy), ldy, P(dw), None, P(ws), n, s)),
        }
        nominal = 2.0 * 64 * O * (C // G) * D * KS * KS / 1e6
        issued = issued_mflop(D, C, O, G, KS)
        for direction, fns in pairs.items():
            for fn in fns:
                for _ in range(3):
                    fn()
            (dm, dlo, dhi), (mm, mlo, mhi) = timed_ab(fns, k)
            verdict = "mfma wholly below direct" if mhi < dlo else "RANGES OVERLAP" if mlo <= dhi else "direct below mfma"
            print(f"  {l1} bands {name} D={D} {direction}: direct median {dm:.4f} ms (min {dlo:.4f}, max {dhi:.4f}), mfma "
                  f"median {mm:.4f} ms (min {mlo:.4f}, max {mhi:.4f}), {nominal:.2f} MFLOP/patch nominal, "
                  f"{issued[direction]:.2f} issued, mfma at {100.0 * nominal * 1e6 * B / (mlo * 1e-3) / PEAK_FP32_MFMA:.2f}% "
                  f"of the fp32 MFMA peak (direct {100.0 * nominal * 1e6 * B / (dlo * 1e-3) / PEAK_FP32_MFMA:.2f}%): "
                  f"{verdict}", flush=True)


def verdict_line(l1, name, direction, direct, new, nominal, issued):
    (dm, dlo, dhi), (mm, mlo, mhi) = direct, new
    verdict = "mfma wholly below direct" if mhi < dlo else "RANGES OVERLAP" if mlo <= dhi else "direct below mfma"
    print(f"  {l1} bands {name} {direction}: direct median {dm:.4f} ms (min {dlo:.4f}, max {dhi:.4f}), mfma "
          f"median {mm:.4f} ms (min {mlo:.4f}, max {mhi:.4f}), {nominal:.2f} MFLOP/patch nominal, "
          f"{issued:.2f} issued, mfma at {100.0 * nominal * 1e6 * B / (mlo * 1e-3) / PEAK_FP32_MFMA:.2f}% "
          f"of the fp32 MFMA peak (direct {100.0 * nominal * 1e6 * B / (dlo * 1e-3) / PEAK_FP32_MFMA:.2f}%): "
          f"{verdict}", flush=True)


SPECTRAL_TAPS = (1, 3, 5, 11)
CONV1_CHUNK = 4                  # VC_MHST_CONV1_CHUNK


def front_sites(l1, k):
    """hsi_encoder.conv1 and the four spectral convolutions, each direction, the direct family (the spectral site: its
    four launches together, as the program issues them) and the MFMA families interleaved; issued MFLOP by
    csrc/mhst_sconv.hip's own loop structure"""
    from vitcnn_amd._lib import lib
    L = lib()
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    D1 = (l1 + 2) // 3
    M3 = B * D1 * 64
    P = lambda t: t.data_ptr()   # noqa: E731
    # conv1: fwd issues 27 steps for each of the chunk's depths (a last chunk that is not full included), wgrad 7 tap
    # tiles per k-step of 4 positions
    x1 = torch.rand(B, l1, 8, 8, device=dev)
    w1, b1, dw1, db1 = (torch.rand(n, device=dev) - 0.5 for n in (16 * 99, 16, 16 * 99, 16))
    y, dy = torch.empty(M3, 16, device=dev), torch.rand(M3, 16, device=dev)
    n1 = L.vc_mhst_conv1_ws_floats(B, l1)
    ws1 = torch.empty(n1, device=dev)
    d1 = (l1, 8, 8, 1, 16, 1, 11, 3, 3, 5, D1)
    pairs = {
        "fwd": (lambda: L.vc_mhst_conv_fwd(B, *d1, P(x1), 1, P(w1), P(b1), P(y), 16, s),
                lambda: L.vc_mhst_conv1_fwd(B, l1, P(x1), P(w1), P(b1), P(y), 16, P(ws1), n1, s)),
        "wgrad": (lambda: L.vc_mhst_conv_wgrad(B, *d1, P(x1), 1, P(dy), 16, P(dw1), P(db1), s),
                  lambda: L.vc_mhst_conv1_wgrad(B, l1, P(x1), P(dy), 16, P(dw1), P(db1), P(ws1), n1, s)),
    }
    nominal = 2.0 * D1 * 64 * 16 * 99 / 1e6
    chunks = (D1 + CONV1_CHUNK - 1) // CONV1_CHUNK
    issued = {"fwd": chunks * CONV1_CHUNK * 4 * 27 * MFMA_FLOP / 1e6, "wgrad": D1 * 16 * 7 * MFMA_FLOP / 1e6}
    for direction, fns in pairs.items():
        for fn in fns:
            for _ in range(3):
                fn()
        direct, new = timed_ab(fns, k)
        verdict_line(l1, f"hsi conv1 D1={D1}", direction, direct, new, nominal, issued[direction])
    # spectral: a (depth, offset) pair inside the cube costs 16 MFMAs per plane in every direction
    x, dx = torch.rand(M3, 16, device=dev), torch.zeros(M3, 16, device=dev)
    ws_, bs_ = [torch.rand(64 * t, device=dev) - 0.5 for t in SPECTRAL_TAPS], [torch.rand(4, device=dev) for _ in SPECTRAL_TAPS]
    dws, dbs = [torch.empty(64 * t, device=dev) for t in SPECTRAL_TAPS], [torch.empty(4, device=dev) for _ in SPECTRAL_TAPS]
    n2 = L.vc_mhst_sconv_ws_floats(B, D1)
    ws2 = torch.empty(n2, device=dev)
    shp = [(D1, 8, 8, 16, 4, 1, t, 1, 1, t // 2, D1) for t in SPECTRAL_TAPS]

    def direct_fwd():
        for i in range(4):
            L.vc_mhst_conv_fwd(B, *shp[i], P(x), 16, P(ws_[i]), P(bs_[i]), P(y) + 16 * i, 16, s)

    def direct_dgrad():
        for i in range(4):
            L.vc_mhst_conv_dgrad(B, *shp[i], P(dy) + 16 * i, 16, P(ws_[i]), P(dx), 16, 1.0 if i else 0.0, s)

    def direct_wgrad():
        for i in range(4):
            L.vc_mhst_conv_wgrad(B, *shp[i], P(x), 16, P(dy) + 16 * i, 16, P(dws[i]), P(dbs[i]), s)

    wp, bp = [P(t) for t in ws_], [P(t) for t in bs_]
    pairs = {
        "fwd": (direct_fwd, lambda: L.vc_mhst_sconv_fwd(B, D1, P(x), 16, *wp, *bp, P(y), 16, P(ws2), n2, s)),
        "dgrad": (direct_dgrad, lambda: L.vc_mhst_sconv_dgrad(B, D1, P(dy), 16, *wp, P(dx), 16, 0.0, P(ws2), n2, s)),
        "wgrad": (direct_wgrad, lambda: L.vc_mhst_sconv_wgrad(B, D1, P(x), 16, P(dy), 16, *(P(t) for t in dws),
                                                              *(P(t) for t in dbs), P(ws2), n2, s)),
    }
    nominal = 2.0 * D1 * 64 * 16 * 4 * sum(SPECTRAL_TAPS) / 1e6
    inside = sum(1 for e in range(D1) for t in range(-5, 6) if 0 <= e + t < D1)
    issued = inside * 16 * MFMA_FLOP / 1e6
    for direction, fns in pairs.items():
        for fn in fns:
            for _ in range(3):
                fn()
        direct, new = timed_ab(fns, k)
        verdict_line(l1, f"hsi spectral D={D1} (direct: 4 launches)", direction, direct, new, nominal, issued)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--") or a == "--conv"]
    conv = "direct"
    if "--conv" in args:
        i = args.index("--conv")
        conv = args[i + 1]
        del args[i:i + 2]
    if conv not in ("direct", "mfma", "mfma_all", "both"):
        raise SystemExit("--conv takes direct, mfma, mfma_all or both")
    k = int(args[0]) if args else 30
    for l1 in (144, 30):
        run(l1, k, "--no-profile" not in sys.argv, ("direct", "mfma", "mfma_all") if conv == "both" else (conv,))
        conv_alone(l1, k)
        pconv_sites(l1, k, fixed_sites=l1 == 144)
        front_sites(l1, k)


if __name__ == "__main__":
    main()
