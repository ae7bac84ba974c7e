"""GPU tool: one device-side PCA `fit` plus `transform` at the Houston2013 shape (349 x 1905 pixels, 144 bands, K = 30) on
a synthetic cube -- 40 planted directions with standard deviations 0.85**j, noise 1e-3, band offsets in [10, 11), made
on the device from a seed.  Prints the times of the three kernels' entry points (device events), of the whole `fit`
(host clock to the end of numpy's eigh: upload excluded, the cube is already on the device) and of `transform`, each
device time also as a multiple of its floor, bytes read / 8 TB/s; then scikit-learn's PCA(K, whiten=True).fit_transform
of the same cube on the host, if scikit-learn is installed, and the whiteness of both outputs.
usage: python tools/pca_fit.py [REPS] [W H C K]"""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vit-cnn_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vitcnn_amd._lib import lib  # noqa: E402
from vitcnn_amd.pca import PCA, cov_workspace_bytes, slab_rows  # noqa: E402

HBM = 8e12   # bytes / s, the MI355X's peak HBM rate


def cube(W, H, C, dev, rank=40, ratio=0.85, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = min(rank, C)
    q, _ = torch.linalg.qr(torch.randn(C, r, generator=g, device=dev, dtype=torch.float64))
    std = ratio ** torch.arange(r, device=dev, dtype=torch.float64)
    x = (torch.randn(W * H, r, generator=g, device=dev, dtype=torch.float64) * std) @ q.T
    x += 1e-3 * torch.randn(W * H, C, generator=g, device=dev, dtype=torch.float64)
    x += 10.0 + torch.rand(C, generator=g, device=dev, dtype=torch.float64)
    return x.to(torch.float32).reshape(W, H, C).contiguous()


def timed(fn, reps, dev):
    """median device time of fn() in ms over `reps` calls, each between two events, after two warm-up calls"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def main(argv):
    reps = int(argv[0]) if argv else 20
    W, H, C, K = (int(a) for a in argv[1:5]) if len(argv) >= 5 else (349, 1905, 144, 30)
    dev = torch.device("cuda", 0)
    L = lib()
    x = cube(W, H, C, dev)
    n = W * H
    s = torch.cuda.current_stream(dev).cuda_stream
    ws = torch.empty(cov_workspace_bytes(n, C), dtype=torch.uint8, device=dev)
    mean = torch.empty(C, dtype=torch.float64, device=dev)
    cov = torch.empty(C, C, dtype=torch.float64, device=dev)
    p = PCA(K).fit(x)
    mean32, wt = p._device_state(dev)
    y = torch.empty(W, H, K, device=dev)
    read = n * C * 4
    floor_ms = read / HBM * 1e3
    print(f"cube {W} x {H} x {C} fp32 ({read / 1e6:.1f} MB), K = {K}, R = {slab_rows()}, workspace {ws.numel() / 1e6:.1f} MB, "
          f"floor = bytes read / 8 TB/s = {floor_ms * 1e3:.1f} us")
    res = {"shape": [W, H, C, K], "floor_us": floor_ms * 1e3}
    for name, fn in (("vc_pca_mean", lambda: L.vc_pca_mean(n, C, C, x.data_ptr(), ws.data_ptr(), mean.data_ptr(), s)),
                     ("vc_pca_cov", lambda: L.vc_pca_cov(n, C, C, x.data_ptr(), mean32.data_ptr(), ws.data_ptr(),
                                                         cov.data_ptr(), s)),
                     ("vc_pca_project", lambda: L.vc_pca_project(n, C, C, K, x.data_ptr(), mean32.data_ptr(),
                                                                 wt.data_ptr(), y.data_ptr(), K, s)),
                     ("PCA.transform", lambda: p.transform(x))):
        med, lo, hi = timed(fn, reps, dev)
        print(f"{name:16s} median {med * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})  = {med / floor_ms:6.2f} x floor")
        res[name + "_us"] = med * 1e3
    fits = []
    for _ in range(max(3, reps // 4)):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        PCA(K).fit(x)
        fits.append((time.perf_counter() - t0) * 1e3)
    print(f"PCA.fit          median {statistics.median(fits):9.3f} ms host clock (kernels + one copy of {C + C * C} doubles + "
          f"numpy eigh), min {min(fits):.3f}, max {max(fits):.3f}")
    res["fit_ms"] = statistics.median(fits)
    try:
        from sklearn.decomposition import PCA as SK
    except ImportError:
        print("scikit-learn: not installed here, host time not measured")
    else:
        host = x.reshape(n, C).cpu().numpy()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref = SK(n_components=K, whiten=True).fit_transform(host)
            ts.append(time.perf_counter() - t0)
        print(f"scikit-learn PCA({K}, whiten=True).fit_transform on the host: median {statistics.median(ts):.3f} s")
        res["sklearn_s"] = statistics.median(ts)
        # whiteness ||Y^T Y / (n - 1) - I||_2 of both outputs, in float64 (scikit-learn computes in the cube's fp32)
        got = p.transform(x).reshape(n, K).cpu().numpy().astype(np.float64)
        for name, out in (("device", got), ("scikit-learn", ref.astype(np.float64))):
            out = out - out.mean(axis=0)
            print(f"whiteness of the {name} output: {np.linalg.norm(out.T @ out / (n - 1) - np.eye(K), 2):.3e}")
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])
