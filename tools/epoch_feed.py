"""GPU tool: what the training feed costs per epoch with the augmentation decisions drawn on the host or on the device
and with the per-epoch reshuffle (DESIGN.md section 33 records the output; nothing here is gated).

Set-up: a Houston2013-size synthetic scene (349 x 1905, 144 + 1 bands) with 2,832 labelled training pixels, ViT-CNN as
get_model builds it, B = 64, P = 9, flip + radiation + mixture augmentation on.  Legs, in one process and alternating:
  (a) draws="host"      PatchBatcher.decisions() per batch and three uploads
  (b) draws="device"    vc_aug_draw per batch
  (c) (b) plus shuffle="epoch": one vc_epoch_shuffle per pass
Each leg is timed twice per round: one pass over the batcher alone (host clock around the pass, ended by a device
synchronise; the time until the last batch is enqueued is recorded as well: that is how long the host is held), and
one train() epoch (train.last_stats' epoch seconds, which include the epoch's checkpoint write).  One warm-up round,
then --epochs timed rounds.  Also: decisions(64) on the host alone, and vc_epoch_shuffle at N = 2,832 and N = 131,072
(device events).
usage: python tools/epoch_feed.py [--epochs 7] [--out profiles/epoch_feed.log]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vit-cnn_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vitcnn_amd import model_utils as mu  # noqa: E402
from vitcnn_amd._lib import lib  # noqa: E402
from vitcnn_amd.window import SHUFFLE_MAX, PatchBatcher  # noqa: E402

LEGS = (("a", "draws=host", dict()),
        ("b", "draws=device", dict(draws="device")),
        ("c", "draws=device, shuffle=epoch", dict(draws="device", shuffle="epoch")))
N_TRAIN, P, B = 2832, 9, 64


def scene(dev):
    rng = np.random.default_rng(0)
    W, H = 349, 1905
    img1 = torch.rand(W, H, 144, device=dev, generator=torch.Generator(dev).manual_seed(1))
    img2 = torch.rand(W, H, 1, device=dev, generator=torch.Generator(dev).manual_seed(2))
    gt = np.zeros((W, H), dtype=np.int64)
    xs, ys = np.meshgrid(np.arange(P // 2 + 1, W - P // 2), np.arange(P // 2 + 1, H - P // 2), indexing="ij")
    pick = rng.choice(xs.size, N_TRAIN, replace=False)
    gt[xs.reshape(-1)[pick], ys.reshape(-1)[pick]] = rng.integers(1, 16, size=N_TRAIN)
    return img1, img2, gt


def spread(ts):
    return f"median {statistics.median(ts):8.3f}  min {min(ts):8.3f}  max {max(ts):8.3f}  ms   (n = {len(ts)})"


def shuffle_ms(N, dev, reps):
    corners = torch.randint(0, 1000, (N, 2), dtype=torch.int32, device=dev)
    labels = torch.randint(0, 16, (N,), dtype=torch.int64, device=dev)
    co, lo = torch.empty_like(corners), torch.empty_like(labels)
    s = torch.cuda.current_stream(dev).cuda_stream

    def launch(e):
        lib().vc_epoch_shuffle(N, 12345, e, 0, 1, 64, corners.data_ptr(), labels.data_ptr(), co.data_ptr(),
                               lo.data_ptr(), None, s)

    launch(0)
    torch.cuda.synchronize(dev)
    ts = []
    for e in range(1, reps + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        launch(e)
        t1.record()
        t1.synchronize()
        ts.append(t0.elapsed_time(t1))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=7, help="timed rounds per leg (after one warm-up round)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "epoch_feed.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("epoch_feed.py measures on a ROCm device; none is visible")
    dev = torch.device("cuda", 0)
    out_path = os.path.abspath(args.out)
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    img1, img2, gt = scene(dev)
    feeds, trains = {}, {}
    for tag, _, kw in LEGS:
        common = dict(ignored_labels=(0,), batch_size=B, flip_augmentation=True, radiation_augmentation=True,
                      mixture_augmentation=True, device=dev, seed=3)
        feeds[tag] = PatchBatcher(img1, img2, gt, P, **common, **kw)
        torch.manual_seed(0)
        net, opt, crit, hp = mu.get_model("Multimodality_Mamba", n_classes=16, n_bands=(144, 1), ignored_labels=[0],
                                          dataset="synthetic", device=dev)
        trains[tag] = (net, opt, crit, PatchBatcher(img1, img2, gt, P, **common, **kw))
    n = len(feeds["a"].centers)
    assert n == N_TRAIN, n
    say(f"epoch feed: {torch.cuda.get_device_name(dev)}, scene 349 x 1905 x (144 + 1), {n} training pixels, "
        f"B = {B} ({len(feeds['a'])} batches per epoch), P = {P}, flip + radiation + mixture, "
        f"1 warm-up + {args.epochs} timed rounds, legs alternating")

    cwd = os.getcwd()
    tmp = tempfile.TemporaryDirectory(prefix="epoch_feed_")   # train() writes checkpoints into the cwd
    os.chdir(tmp.name)
    feed_ms = {t: [] for t, _, _ in LEGS}
    held_ms = {t: [] for t, _, _ in LEGS}
    train_ms = {t: [] for t, _, _ in LEGS}
    launch = {}
    try:
        for rnd in range(args.epochs + 1):
            for tag, _, _ in LEGS:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _batch in feeds[tag]:
                    pass
                t1 = time.perf_counter()
                torch.cuda.synchronize(dev)
                t2 = time.perf_counter()
                if rnd:
                    feed_ms[tag].append((t2 - t0) * 1e3)
                    held_ms[tag].append((t1 - t0) * 1e3)
            for tag, _, _ in LEGS:
                net, opt, crit, loader = trains[tag]
                mu.train("feed_" + tag, 0, None, net, opt, crit, loader, 1, display_iter=0, device=dev)
                torch.cuda.synchronize(dev)
                st = mu.train.last_stats
                launch[tag] = st["launch"]
                if rnd:
                    train_ms[tag].append(st["epochs"][0]["seconds"] * 1e3)
    finally:
        os.chdir(cwd)
        tmp.cleanup()

    say()
    say("one pass over the batcher alone, per epoch (host clock, ended by a device synchronise):")
    for tag, name, _ in LEGS:
        say(f"  ({tag}) {name:30s} {spread(feed_ms[tag])}")
    say("  of which until the last batch is enqueued (the host is held this long):")
    for tag, name, _ in LEGS:
        say(f"  ({tag}) {name:30s} {spread(held_ms[tag])}")
    say()
    say("one train() epoch (train.last_stats seconds: the steps, the loss read-back and the checkpoint write):")
    for tag, name, _ in LEGS:
        say(f"  ({tag}) {name:30s} {spread(train_ms[tag])}   launch: {launch[tag]}")

    host = feeds["a"]
    ts = []
    for _ in range(200):
        t0 = time.perf_counter()
        host.decisions(B)
        ts.append((time.perf_counter() - t0) * 1e3)
    say()
    say(f"PatchBatcher.decisions({B}) on the host alone, per batch:   {spread(ts)}")
    say()
    say("vc_epoch_shuffle, one launch (device events):")
    for N, reps in ((N_TRAIN, 20), (SHUFFLE_MAX, 5)):
        say(f"  N = {N:7d}: {spread(shuffle_ms(N, dev, reps))}")

    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
