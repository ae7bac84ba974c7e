"""GPU tool: the end of a run (main.py:500-519) on a synthetic Houston2013-shaped scene -- 349 x 1905 pixels, 144 + 1
bands, 15 labelled classes on about 15k pixels drawn from a seeded generator (the rest: ignored label 0) -- with
ViT-CNN at its defaults (9 x 9 windows, 16 outputs) and hash-filled weights.  In one process, alternating, it times

  (a) the flow before evaluate(): test() over every in-scene window, the float64 [W, H, 16] map copied to the host,
      np.argmax there, metrics() (which uploads the class map again);
  (b) evaluate(): only the windows centred on labelled pixels, class map and confusion counts on the device;
  (c) evaluate() with border="symmetric": the same with windows over the scene's edges mirrored.

Each leg runs once to warm up and then REPS times (host clock around the call, which ends in a device-to-host copy;
the cubes are on the device before the clock starts, for every leg); median and range are printed.  (a) and (b) must
return the same confusion matrix: that is asserted.  The log goes to stdout and to --log.
usage: python tools/evaluate_scene.py [REPS] [--log PATH] [--size W H]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vit-cnn_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vitcnn_amd import model_utils as mu  # noqa: E402
from vitcnn_amd.hashinit import fill_module_  # noqa: E402
from vitcnn_amd.metrics import metrics  # noqa: E402

N_CLASSES, LABELLED = 16, 15000


def scene(W, H, dev, seed=0):
    """(hsi [W, H, 144], lidar [W, H, 1]) fp32 on the device and gt [W, H] int64 on the host: 15 classes in a 3 x 5
    grid of regions with their own band profiles (so the predicted class varies over the scene), `LABELLED` pixels
    of them labelled with their region's class, anywhere in the scene, edges included"""
    g = torch.Generator(device=dev).manual_seed(seed)
    xx, yy = torch.meshgrid(torch.arange(W, device=dev), torch.arange(H, device=dev), indexing="ij")
    region = (xx * 3 // W) * 5 + (yy * 5 // H)
    prof = torch.rand(15, 144, generator=g, device=dev)
    hsi = 0.7 * prof[region] + 0.3 * torch.rand(W, H, 144, generator=g, device=dev)
    lidar = region[..., None] / 15.0 + 0.1 * torch.rand(W, H, 1, generator=g, device=dev)
    rng = np.random.default_rng(seed)
    gt = np.zeros(W * H, dtype=np.int64)
    pick = rng.choice(W * H, size=min(LABELLED, W * H // 2), replace=False)
    gt[pick] = region.reshape(-1).cpu().numpy()[pick] + 1
    return hsi.contiguous(), lidar.float().contiguous(), gt.reshape(W, H)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reps", nargs="?", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "evaluate_scene.log"))
    ap.add_argument("--size", nargs=2, type=int, default=(349, 1905))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_scene.py measures on the GPU; there is none here (not measured)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    W, H = args.size
    hsi, lidar, gt = scene(W, H, dev)
    model, _, _, hp = mu.get_model("Multimodality_Mamba", n_classes=N_CLASSES, n_bands=(144, 1), ignored_labels=[0],
                                   dataset="synthetic", device=dev)
    fill_module_(model)
    hp["test_stride"] = 1
    hpb = dict(hp, border="symmetric")
    P = hp["patch_size"]
    labelled = int((gt != 0).sum())
    inside = int((gt[P // 2:W - P // 2, P // 2:H - P // 2] != 0).sum())
    say(f"scene {W} x {H}, 144 + 1 bands, P = {P}: {(W - P + 1) * (H - P + 1)} in-scene windows, {labelled} labelled "
        f"pixels ({inside} with an in-scene window, {labelled - inside} within {P // 2} of an edge)")

    def leg_a():
        probs = mu.test(0, model, hsi, lidar, hp)
        return metrics(np.argmax(probs, axis=-1), gt, ignored_labels=hp["ignored_labels"], n_classes=N_CLASSES)

    legs = [("a test + host argmax + metrics", leg_a),
            ("b evaluate", lambda: mu.evaluate(0, model, hsi, lidar, gt, hp)),
            ("c evaluate border=symmetric", lambda: mu.evaluate(0, model, hsi, lidar, gt, hpb))]
    last = {name: fn() for name, fn in legs}                  # warm-up: every shape of the timed window
    times = {name: [] for name, _ in legs}
    for _ in range(args.reps):
        for name, fn in legs:                                 # alternating: the legs see the same machine state
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            last[name] = fn()
            times[name].append(time.perf_counter() - t0)
    res = {"shape": [W, H], "labelled": labelled, "reps": args.reps}
    for name, _ in legs:
        t = times[name]
        say(f"({name[0]}) {name[2:]:34s} median {statistics.median(t) * 1e3:10.1f} ms  (min {min(t) * 1e3:.1f}, "
            f"max {max(t) * 1e3:.1f}, {len(t)} runs)   accuracy {last[name]['Accuracy']:.3f} %  kappa "
            f"{last[name]['Kappa']:.4f}")
        res[name[0] + "_ms"] = statistics.median(t) * 1e3
    a, b, c = (last[name] for name, _ in legs)
    say(f"(a) / (b) = {res['a_ms'] / res['b_ms']:.1f}, (a) / (c) = {res['a_ms'] / res['c_ms']:.1f}; windows evaluated "
        f"(a) {(W - P + 1) * (H - P + 1)}, (b) {inside}, (c) {labelled}: ratio (a) / (b) {(W - P + 1) * (H - P + 1) / inside:.1f}")
    same = np.array_equal(a["Confusion matrix"], b["Confusion matrix"])
    say(f"confusion matrix of (a) and (b) equal: {same}; pixels counted {int(a['Confusion matrix'].sum())}, predicted 0 "
        f"(no window) in (b) {int(b['Confusion matrix'][:, 0].sum())}, in (c) {int(c['Confusion matrix'][:, 0].sum())}; "
        f"classes predicted {int((b['Confusion matrix'].sum(0) > 0).sum())}")
    say(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert same, "evaluate() and test() + argmax + metrics() disagree on the confusion matrix"


if __name__ == "__main__":
    main()
