"""The end of a run on the device (main.py:500-519): test() with a mirrored border, run(centers=), predict() and
evaluate() against today's test() on the host-padded scene (utils.padding_image / restore_from_padding,
utils.py:320-354) followed by np.argmax and metrics(); PatchBatcher(border=) against slices of np.pad.

The exact checks use a stub model whose logits are sums of products of small dyadic numbers, exact in fp32 in any
order: whatever the batch grouping, equal windows give equal logits, so every comparison is array-equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ("symmetric", "reflect", "constant")
NCLS = 5


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class Stub(torch.nn.Module):
    """logits[b] = Wc centre spectrum + Ws per-channel window sums, per sample: inputs are integers of magnitude below
    16 and the weights multiples of 1/4 below 4, so every partial sum is a multiple of 1/4 below 2^15 in magnitude --
    exact in fp32"""

    def __init__(self, C, P, ncls=NCLS):
        super().__init__()
        g = torch.Generator().manual_seed(C * 100 + P)
        self.P = P
        self.register_buffer("wc", torch.randint(-15, 16, (ncls, C), generator=g).float() / 4)
        self.register_buffer("ws", torch.randint(-15, 16, (ncls, C), generator=g).float() / 4)

    def forward(self, x1, x2):
        x = torch.cat([x1, x2], dim=1)
        h = self.P // 2
        centre, sums = x[:, :, h, h], x.sum(dim=(2, 3))
        return (centre[:, None, :] * self.wc[None]).sum(-1) + (sums[:, None, :] * self.ws[None]).sum(-1)


W, H = 14, 12
_SCENE = {}


def _scene():
    """14 x 12, 6 + 1 bands of integers in -15..15; labels 0..4 with 0 ignored, all four edges and corners labelled"""
    if not _SCENE:
        rng = np.random.default_rng(31)
        gt = rng.integers(0, NCLS, size=(W, H))
        gt[0, :], gt[-1, :], gt[:, 0], gt[:, -1] = 1, 2, 3, 4
        gt[0, 0], gt[0, -1], gt[-1, 0], gt[-1, -1] = 4, 3, 2, 1
        gt[5, 0] = gt[0, 7] = 0                                   # ignored pixels on an edge too
        _SCENE.update(img1=rng.integers(-15, 16, size=(W, H, 6)).astype(np.float32),
                      img2=rng.integers(-15, 16, size=(W, H, 1)).astype(np.float32), gt=gt)
    return _SCENE["img1"], _SCENE["img2"], _SCENE["gt"]


def _hp(P, stride=1, border=None, ncls=NCLS):
    hp = {"patch_size": P, "n_classes": ncls, "batch_size": 16, "device": DEV, "ignored_labels": [0],
          "test_stride": stride}
    if border is not None:
        hp["border"] = border
    return hp


def _pad(img, P, mode):
    """utils.padding_image (utils.py:339-343)"""
    h = P // 2
    return np.pad(img, [[h, h], [h, h]] + [[0, 0]] * (img.ndim - 2), mode=mode)


def _restore(a, P):
    """utils.restore_from_padding (utils.py:346-354)"""
    h = P // 2
    return a[h:a.shape[0] - h, h:a.shape[1] - h]


_PADDED = {}


def _padded_probs(P, mode, stride):
    """restore_from_padding(test(padding_image(img1), padding_image(img2))) by today's test() (no border), once"""
    key = (P, mode, stride)
    if key not in _PADDED:
        from vitcnn_amd import model_utils as mu
        img1, img2, _ = _scene()
        net = Stub(7, P).to(DEV)
        _PADDED[key] = _restore(mu.test(0, net, _pad(img1, P, mode), _pad(img2, P, mode), _hp(P, stride)), P)
    return _PADDED[key]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", [5, 4])
def test_bordered_test_is_the_padded_run(P, mode, stride):
    """(i) and (vi)"""
    _need_gpu()
    from vitcnn_amd import model_utils as mu
    img1, img2, gt = _scene()
    net = Stub(7, P).to(DEV)
    got = mu.test(0, net, img1, img2, _hp(P, stride, mode))
    want = _padded_probs(P, mode, stride)
    assert got.dtype == np.float64 and got.shape == (W, H, NCLS) == want.shape
    assert np.array_equal(got, want)
    if stride == 1:
        assert got.any(-1).all()                        # every pixel has a window
        edge = np.zeros((W, H), dtype=bool)
        edge[:P // 2], edge[W - P // 2:], edge[:, :P // 2], edge[:, H - P // 2:] = True, True, True, True
        assert (edge & (gt != 0)).sum() > 40 and got[edge & (gt != 0)].any(-1).all()
        plain = mu.test(0, net, img1, img2, _hp(P, 1))
        assert not plain[0].any() and not plain[:, 0].any()     # which today's run leaves at zero
        hit = plain.any(-1)
        assert hit.sum() == (W - P + 1) * (H - P + 1) and np.array_equal(got[hit], plain[hit])   # in-scene windows


@pytest.mark.parametrize("border", [None, "symmetric"])
@pytest.mark.parametrize("P,stride", [(5, 1), (4, 1), (5, 2)])
def test_run_at_centres_is_the_full_run_there(P, stride, border):
    """(ii): also centres given twice, off the scene and between strides"""
    _need_gpu()
    from vitcnn_amd.window import SlidingWindowInference
    img1, img2, gt = _scene()
    net = Stub(7, P).to(DEV)
    runner = SlidingWindowInference(net, img1, img2, P, step=stride, n_classes=NCLS, device=DEV, border=border)
    full = runner.run(batch_size=16)
    c = np.argwhere(gt != 0)
    c = np.concatenate([c[::-1], c[:5], [[-1, 3], [W, 0], [2, H]]])
    got = runner.run(batch_size=16, centers=c)
    sel = np.zeros((W, H), dtype=bool)
    sel[gt != 0] = True
    assert np.array_equal(got[sel], full[sel]) and not got[~sel].any()
    assert full[sel].any() and (border is None or stride > 1 or full[sel].any(-1).all())
    assert not runner.run(centers=np.zeros((0, 2), dtype=np.int64)).any()
    with pytest.raises(ValueError, match="centers"):
        runner.run(centers=np.zeros((3, 2)))


@pytest.mark.parametrize("border", [None, "symmetric", "constant"])
@pytest.mark.parametrize("P", [5, 4])
def test_predict_is_argmax_of_test(P, border):
    """(iii)"""
    _need_gpu()
    from vitcnn_amd import model_utils as mu
    img1, img2, gt = _scene()
    net = Stub(7, P).to(DEV)
    hp = _hp(P, 1, border)
    want = np.argmax(mu.test(0, net, img1, img2, hp), -1)
    got = mu.predict(0, net, img1, img2, hp)
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (W, H)
    assert np.array_equal(got.cpu().numpy(), want) and len(np.unique(want)) > 2
    c = np.argwhere(gt != 0)
    part = mu.predict(0, net, img1, img2, hp, centers=c).cpu().numpy()
    assert np.array_equal(part[gt != 0], want[gt != 0]) and not part[gt == 0].any()


def _same_dict(a, b):
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k
    assert a["Confusion matrix"].dtype == b["Confusion matrix"].dtype


@pytest.mark.parametrize("P", [5, 4])
def test_evaluate_is_test_argmax_metrics(P):
    """(iv) without a border: labelled pixels with no in-scene window count as predicted 0, as they do today;
    (v) with one: the same flow over the padded scene after restoring"""
    _need_gpu()
    from vitcnn_amd import model_utils as mu
    from vitcnn_amd.metrics import metrics
    img1, img2, gt = _scene()
    net = Stub(7, P).to(DEV)
    hp = _hp(P, 1)
    want = metrics(np.argmax(mu.test(0, net, img1, img2, hp), -1), gt, ignored_labels=[0], n_classes=NCLS)
    got = mu.evaluate(0, net, img1, img2, gt, hp)
    _same_dict(got, want)
    assert got["Confusion matrix"].sum() == (gt != 0).sum() and got["Confusion matrix"][:, 0].sum() > 40
    wantb = metrics(np.argmax(_padded_probs(P, "symmetric", 1), -1), gt, ignored_labels=[0], n_classes=NCLS)
    gotb = mu.evaluate(0, net, img1, img2, gt, _hp(P, 1, "symmetric"))
    _same_dict(gotb, wantb)
    assert not np.array_equal(gotb["Confusion matrix"], got["Confusion matrix"])


_REAL = {}


def _real():
    """Multimodality_Mamba at P = 7, 8 + 1 bands, 5 classes, hash-filled; a 12 x 10 scene; today's test() on the
    host-padded scene, restored"""
    if not _REAL:
        from vitcnn_amd import Multimodality_Mamba
        from vitcnn_amd import model_utils as mu
        from vitcnn_amd.hashinit import fill_module_
        P = 7
        net = Multimodality_Mamba(P, 1, 1, 8, 1, 32, NCLS, "multi_clock_gate")
        fill_module_(net)
        net = net.to(DEV)
        rng = np.random.default_rng(12)
        img1 = rng.random((12, 10, 8), dtype=np.float32)
        img2 = rng.random((12, 10, 1), dtype=np.float32)
        ref = _restore(mu.test(0, net, _pad(img1, P, "symmetric"), _pad(img2, P, "symmetric"), _hp(P, 1)), P)
        _REAL.update(net=net, img1=img1, img2=img2, ref=ref, P=P)
    return _REAL


def test_real_model_bordered_and_centres():
    """the bordered probabilities and the centers= probabilities against today's test() on the host-padded scene:
    the same kernels under another batch grouping, within the project's fp32 bound of tests/test_window_gpu.py,
    1e-3 of the largest logit magnitude"""
    _need_gpu()
    from vitcnn_amd import model_utils as mu
    from vitcnn_amd.window import SlidingWindowInference
    r = _real()
    net, img1, img2, ref, P = r["net"], r["img1"], r["img2"], r["ref"], r["P"]
    scale = np.abs(ref).max()
    got = mu.test(0, net, img1, img2, _hp(P, 1, "symmetric"))
    err = np.abs(got - ref).max() / scale
    print(f"PARITY bordered test() vs host-padded test(): {err:.3e} of the largest logit")
    assert got.shape == ref.shape == (12, 10, NCLS) and ref.any(-1).all()
    assert err < 1e-3, err
    rng = np.random.default_rng(5)
    c = np.argwhere(rng.random((12, 10)) < 0.3)
    runner = SlidingWindowInference(net, img1, img2, P, step=1, n_classes=NCLS, device=DEV, border="symmetric")
    part = runner.run(batch_size=16, centers=c)
    sel = np.zeros((12, 10), dtype=bool)
    sel[c[:, 0], c[:, 1]] = True
    errc = np.abs(part[sel] - ref[sel]).max() / scale
    print(f"PARITY centers= run vs host-padded test(): {errc:.3e} of the largest logit")
    assert errc < 1e-3 and not part[~sel].any()
    # without a border: the centres that have an in-scene window, against today's full run
    plain = mu.test(0, net, img1, img2, _hp(P, 1))
    partp = SlidingWindowInference(net, img1, img2, P, step=1, n_classes=NCLS, device=DEV).run(batch_size=16, centers=c)
    hit = sel & plain.any(-1)
    errp = np.abs(partp[hit] - plain[hit]).max() / np.abs(plain).max()
    print(f"PARITY centers= run vs full run, no border: {errp:.3e} of the largest logit")
    assert hit.any() and errp < 1e-3 and not partp[~hit].any()


def _np_xform(p, code):
    """datasets.py flip / rotate on a [P, P, C] patch"""
    if code & 3:
        if code & 1:
            p = np.fliplr(p)
        if code & 2:
            p = np.flipud(p)
    elif code >> 2:
        p = np.rot90(p, k=code >> 2)
    return p


def test_patch_batcher_border_yields_np_pad_slices():
    _need_gpu()
    from vitcnn_amd.window import PatchBatcher
    img1, img2, gt = _scene()
    P, h = 5, 2
    kw = dict(ignored_labels=[0], batch_size=32, flip_augmentation=True, device=DEV, seed=3)
    pb = PatchBatcher(img1, img2, gt, P, border="symmetric", **kw)
    twin = PatchBatcher(img1, img2, gt, P, border="symmetric", **kw)      # the same host draws
    assert sorted(map(tuple, pb.centers.tolist())) == sorted(map(tuple, np.argwhere(gt != 0).tolist()))
    assert int(pb.corners.min()) == -h
    p1, p2 = _pad(img1, P, "symmetric"), _pad(img2, P, "symmetric")
    seen, rotated = 0, 0
    for x1, x2, t in pb:
        n = x1.shape[0]
        codes = twin.decisions(n)[0]
        cen = pb.centers[seen:seen + n]
        assert np.array_equal(t.cpu().numpy(), gt[cen[:, 0], cen[:, 1]])
        w1 = np.stack([_np_xform(p1[x:x + P, y:y + P], c).transpose(2, 0, 1) for (x, y), c in zip(cen, codes)])
        w2 = np.stack([_np_xform(p2[x:x + P, y:y + P], c).transpose(2, 0, 1) for (x, y), c in zip(cen, codes)])
        assert np.array_equal(x1.cpu().numpy(), w1) and np.array_equal(x2.cpu().numpy(), w2)
        seen += n
        rotated += int((codes != 0).sum())
    assert seen == len(pb.centers) == (gt != 0).sum() and rotated > 10


def test_patch_batcher_border_mixture_label_window_is_the_mirrored_map():
    _need_gpu()
    from vitcnn_amd.window import PatchBatcher
    img1, img2, gt = _scene()
    P, h, n = 5, 2, 24
    pb = PatchBatcher(img1, img2, gt, P, ignored_labels=[0], batch_size=32, flip_augmentation=True, device=DEV, seed=4,
                      mixture_augmentation=True, border="symmetric")
    near = np.argsort(np.minimum.reduce([pb.centers[:, 0], W - 1 - pb.centers[:, 0], pb.centers[:, 1],
                                         H - 1 - pb.centers[:, 1]]), kind="stable")[:n]     # the centres nearest an edge
    cor = pb.corners[torch.as_tensor(near).to(DEV)].contiguous()
    codes = np.array([0, 1, 2, 3, 4, 8, 12, 0] * 3, dtype=np.uint8)
    xd = torch.from_numpy(codes).to(DEV)
    x1 = torch.zeros(n, 6, P, P, device=DEV)
    mix = np.tile(np.array([[0.5, 0.25]], dtype=np.float32), (n, 1))
    pb.apply_noise(x1, cor, xd.data_ptr(), np.zeros(n, dtype=np.float32), mix, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    lab = pb._last_noise[2].cpu().numpy().reshape(n, P, P)
    pg = _pad(gt, P, "symmetric")
    for i, k in enumerate(near):
        x, y = pb.centers[k]
        assert np.array_equal(lab[i], _np_xform(pg[x:x + P, y:y + P, None], codes[i])[:, :, 0].astype(np.float32))
    assert int(cor.min()) == -h and torch.isfinite(x1).all()
    for a, b, t in pb:                                   # and whole batches iterate with the noise on
        assert torch.isfinite(a).all() and torch.isfinite(b).all()


def test_patch_batcher_without_border_is_unchanged():
    """no `border` argument: the reference's edge filter and the plain gather, as before -- two instances with one
    seed yield the same batches, and those are the unpadded windows"""
    _need_gpu()
    from vitcnn_amd.window import PatchBatcher
    img1, img2, gt = _scene()
    P, p = 5, 2
    kw = dict(ignored_labels=[0], batch_size=32, flip_augmentation=True, device=DEV, seed=3)
    a, b, twin = (PatchBatcher(img1, img2, gt, P, **kw) for _ in range(3))
    assert a.border == 0
    xs, ys = np.nonzero(gt != 0)
    keep = (xs > p) & (xs < W - p) & (ys > p) & (ys < H - p)
    assert sorted(map(tuple, a.centers.tolist())) == sorted(zip(xs[keep].tolist(), ys[keep].tolist()))
    seen = 0
    for (x1, x2, t), (y1, y2, u) in zip(a, b):
        assert torch.equal(x1, y1) and torch.equal(x2, y2) and torch.equal(t, u)
        codes = twin.decisions(x1.shape[0])[0]
        cen = a.centers[seen:seen + x1.shape[0]]
        w1 = np.stack([_np_xform(img1[x - p:x - p + P, y - p:y - p + P], c).transpose(2, 0, 1)
                       for (x, y), c in zip(cen, codes)])
        assert np.array_equal(x1.cpu().numpy(), w1)
        seen += x1.shape[0]
    assert seen == len(a.centers) == keep.sum()


def test_train_and_val_over_the_bordered_batcher(tmp_path, monkeypatch):
    """one epoch of train() and val() over every labelled pixel of the small scene with the real model"""
    _need_gpu()
    from vitcnn_amd import AdamW, CrossEntropyLoss, Multimodality_Mamba
    from vitcnn_amd import model_utils as mu
    from vitcnn_amd.hashinit import fill_module_
    from vitcnn_amd.window import PatchBatcher
    monkeypatch.chdir(tmp_path)
    r = _real()
    rng = np.random.default_rng(8)
    gt = rng.integers(0, NCLS, size=(12, 10))
    gt[0, :], gt[:, -1] = 1, 2
    net = Multimodality_Mamba(r["P"], 1, 1, 8, 1, 32, NCLS, "multi_clock_gate")
    fill_module_(net)
    net = net.to(DEV)
    loader = PatchBatcher(r["img1"], r["img2"], gt, r["P"], ignored_labels=[0], batch_size=64, flip_augmentation=True,
                          device=DEV, border="symmetric")
    assert len(loader.centers) == (gt != 0).sum() > 64
    w = torch.ones(NCLS)
    w[0] = 0
    best = mu.train("b", 0, None, net, AdamW(net.parameters(), lr=1e-4), CrossEntropyLoss(weight=w.to(DEV)), loader, 1,
                    display_iter=0, device=torch.device(DEV))
    losses = mu.train.last_stats["losses"]
    assert best is not None and len(losses) == len(loader) == 2 and np.isfinite(losses).all()
    acc = mu.val(net, loader, device=DEV)
    assert np.isfinite(acc) and 0.0 <= acc <= 1.0
