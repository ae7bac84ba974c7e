"""PatchBatcher(shuffle="epoch", draws="device") on the GPU: every batch equals the existing gather and noise kernels
fed the host restatements (`epoch_order`, `device_decisions`), passes reshuffle and can be replayed, the shards of a
world of 2 partition every epoch's list, the defaults are unchanged, and train() runs over such a loader."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, H, P, B = 12, 10, 5, 4


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _scene():
    """12 x 10, 3 + 1 bands; the LiDAR band holds the pixel's index x * H + y, so a gathered patch names its centre"""
    rng = np.random.default_rng(4)
    img1 = rng.random((W, H, 3), dtype=np.float32)
    img2 = np.arange(W * H, dtype=np.float32).reshape(W, H, 1)
    gt = rng.integers(0, 4, size=(W, H))
    gt[3, 3] = 0
    inner = gt[3:W - 2, 3:H - 2]             # the centres MultiModalX keeps: P // 2 < x < W - P // 2, likewise y
    if np.count_nonzero(inner) % 2:          # an even list: the two shards of a world of 2 need no padding
        gt[4, 4] = 0 if gt[4, 4] else 1
    return img1, img2, gt


def _batcher(**kw):
    from vitcnn_amd.window import PatchBatcher
    img1, img2, gt = _scene()
    args = dict(ignored_labels=[0], batch_size=B, device=DEV, seed=11, flip_augmentation=True,
                radiation_augmentation=True, mixture_augmentation=True)
    args.update(kw)
    return PatchBatcher(img1, img2, gt, P, **args)


def _centre_ids(x2):
    """pixel indices of the yielded samples, read from the LiDAR patches' centre (flips and rotations keep it)"""
    return x2[:, 0, P // 2, P // 2].round().long().cpu().tolist()


def test_batches_equal_the_kernels_fed_the_host_restatements():
    _need_gpu()
    from vitcnn_amd._lib import lib
    from vitcnn_amd.window import device_decisions, epoch_order
    L = lib()
    _, _, gt = _scene()
    pb = _batcher(shuffle="epoch", draws="device")
    ref = _batcher()                          # the construction-time list, the cubes and the mixture tables
    full = ref.centers
    N = len(full)
    assert N % 2 == 0 and N > 3 * B and len(pb) == -(-N // B)
    s = torch.cuda.current_stream().cuda_stream
    gid, noisy, orders = 0, 0, []
    for e in range(2):
        order = epoch_order(N, pb.seed, e)
        orders.append(order)
        b0 = 0
        for x1, x2, t in pb:
            n = int(t.shape[0])
            assert pb.epoch == e and n == min(B, N - b0)
            cen = full[order[b0:b0 + n]]
            assert np.array_equal(pb.centers[b0:b0 + n], cen)
            cor = torch.from_numpy(np.ascontiguousarray((cen - P // 2).astype(np.int32))).to(DEV)
            codes, rad, mix = device_decisions(pb.noise_seed, gid, n, True, True, True)
            xd = torch.from_numpy(codes).to(DEV)
            r1, r2 = torch.empty(n, 3, P, P, device=DEV), torch.empty(n, 1, P, P, device=DEV)
            L.vc_patch_gather(W, H, 3, P, ref.c1.data_ptr(), cor.data_ptr(), 0, 0, n, xd.data_ptr(), r1.data_ptr(), s)
            L.vc_patch_gather(W, H, 1, P, ref.c2.data_ptr(), cor.data_ptr(), 0, 0, n, xd.data_ptr(), r2.data_ptr(), s)
            clean = r1.clone()
            ref.gid = gid
            ref.apply_noise(r1, cor, xd.data_ptr(), rad, mix, s)
            torch.cuda.synchronize()
            noisy += int((r1 != clean).flatten(1).any(1).sum())
            assert torch.equal(x1, r1) and torch.equal(x2, r2), (e, b0)
            assert t.dtype == torch.int64 and np.array_equal(t.cpu().numpy(), gt[cen[:, 0], cen[:, 1]])
            assert _centre_ids(x2) == (cen[:, 0] * H + cen[:, 1]).tolist()
            gid += n
            b0 += n
        assert b0 == N
    assert pb.gid == gid == 2 * N
    assert noisy >= 3                         # the noise path was compared on noised samples, not on zeros only
    assert not np.array_equal(orders[0], orders[1])


def test_passes_reshuffle_and_set_epoch_replays():
    _need_gpu()
    pb = _batcher(shuffle="epoch", draws="device")
    passes = [list(pb) for _ in range(2)]     # the yielded tensors themselves, pass 0's kept across pass 1
    ids = [sum((_centre_ids(x2) for _, x2, _ in p), []) for p in passes]
    assert ids[0] != ids[1] and sorted(ids[0]) == sorted(ids[1]) and len(set(ids[0])) == len(ids[0])
    labels = [torch.cat([t for _, _, t in p]).cpu().tolist() for p in passes]
    assert sorted(labels[0]) == sorted(labels[1])
    assert pb.epoch == 1
    # labels handed out by pass 0 were not overwritten by pass 1's shuffle
    _, _, gt = _scene()
    assert labels[0] == [int(gt[i // H, i % H]) for i in ids[0]]
    pb.set_epoch(0)
    pb.gid = 0
    again = list(pb)
    assert pb.epoch == 0 and len(again) == len(passes[0])
    for (a1, a2, at), (b1, b2, bt) in zip(again, passes[0]):
        assert torch.equal(a1, b1) and torch.equal(a2, b2) and torch.equal(at, bt)
    assert [i for _, x2, _ in pb for i in _centre_ids(x2)] == ids[1]      # and the count goes on from there


def test_shards_of_a_world_of_two_partition_every_epoch():
    _need_gpu()
    from vitcnn_amd.window import epoch_order
    whole = _batcher()
    everything = sorted((whole.centers[:, 0] * H + whole.centers[:, 1]).tolist())
    N = len(everything)
    ranks = [_batcher(shuffle="epoch", draws="device", rank=r, world=2) for r in (0, 1)]
    firsts = []
    for e in range(3):
        got = [[i for _, x2, _ in pb for i in _centre_ids(x2)] for pb in ranks]
        assert len(got[0]) == len(got[1]) == N // 2
        assert not set(got[0]) & set(got[1]) and sorted(got[0] + got[1]) == everything
        for r, pb in enumerate(ranks):
            cen = whole.centers[epoch_order(N, pb.seed, e, r, 2)]
            assert got[r] == (cen[:, 0] * H + cen[:, 1]).tolist()
        firsts.append(set(got[0]))
    assert firsts[0] != firsts[1] or firsts[1] != firsts[2]       # samples move between the ranks


def test_defaults_are_unchanged():
    _need_gpu()
    a, b = _batcher(), _batcher(shuffle=None, draws="host")
    whole = 0
    for _ in range(2):
        for (a1, a2, at), (b1, b2, bt) in zip(a, b):
            assert torch.equal(a1, b1) and torch.equal(a2, b2) and torch.equal(at, bt)
            whole += int(at.shape[0])
    assert whole == 2 * len(a.centers) and a.gid == b.gid == whole
    # and the order is the construction-time one in every pass
    ids = [[i for _, x2, _ in a for i in _centre_ids(x2)] for _ in range(2)]
    assert ids[0] == ids[1] == (a.centers[:, 0] * H + a.centers[:, 1]).tolist()


def test_each_option_alone():
    """shuffle="epoch" with host draws keeps decisions()'s stream; draws="device" alone keeps the construction order"""
    _need_gpu()
    from vitcnn_amd.window import device_decisions
    base = _batcher()
    order0 = (base.centers[:, 0] * H + base.centers[:, 1]).tolist()
    dd = _batcher(draws="device", radiation_augmentation=False, mixture_augmentation=False)
    plain = _batcher(flip_augmentation=False, radiation_augmentation=False, mixture_augmentation=False)
    codes = device_decisions(dd.noise_seed, 0, len(order0), True, False, False)[0]
    k = 0
    for (x1, x2, t), (p1, p2, pt) in zip(dd, plain):
        assert _centre_ids(x2) == order0[k:k + len(t)] and torch.equal(t, pt)
        for i in range(len(t)):               # the drawn code applied to the untransformed patch
            c = int(codes[k + i])
            q = p1[i].cpu().numpy().transpose(1, 2, 0)
            if c & 3:
                q = np.fliplr(q) if c & 1 else q
                q = np.flipud(q) if c & 2 else q
            elif c >> 2:
                q = np.rot90(q, k=c >> 2)
            assert np.array_equal(x1[i].cpu().numpy(), np.ascontiguousarray(q.transpose(2, 0, 1)))
        k += len(t)
    sh, host = _batcher(shuffle="epoch"), _batcher()
    got = sum((_centre_ids(x2) for _, x2, _ in sh), [])
    assert sorted(got) == sorted(order0) and got != order0
    host.decisions(len(order0))               # the RandomState stream one pass of host draws consumes
    assert np.array_equal(sh.rng.random_sample(3), host.rng.random_sample(3))


def test_train_over_a_reshuffled_device_drawn_loader(tmp_path, monkeypatch):
    """train() for 2 epochs on ViT-CNN (144 + 1 bands, P = 9, every labelled pixel through the mirrored border) with
    both options on: finite losses, and the step stays one graph replay per batch"""
    _need_gpu()
    from vitcnn_amd import model_utils as mu
    from vitcnn_amd.window import PatchBatcher
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(2)
    img1 = rng.random((W, H, 144), dtype=np.float32)
    img2 = rng.random((W, H, 1), dtype=np.float32)
    gt = rng.integers(0, 5, size=(W, H))
    model, opt, crit, hp = mu.get_model("Multimodality_Mamba", n_classes=5, n_bands=(144, 1), ignored_labels=[0],
                                        dataset="synthetic", device=torch.device(DEV))
    loader = PatchBatcher(img1, img2, gt, 9, ignored_labels=[0], batch_size=16, device=DEV, seed=1,
                          flip_augmentation=True, radiation_augmentation=True, mixture_augmentation=True,
                          border="symmetric", shuffle="epoch", draws="device")
    n = len(loader.centers)
    mu.train("t", 0, None, model, opt, crit, loader, 2, scheduler=hp["scheduler"], display_iter=0,
             device=torch.device(DEV))
    st = mu.train.last_stats
    assert st["launch"] == "hipGraph", st["launch"]
    assert len(st["losses"]) == 2 * len(loader) and all(np.isfinite(v) for v in st["losses"])
    assert [ep["patches"] for ep in st["epochs"]] == [n, n]
    assert loader.epoch == 1 and loader.gid == 2 * n
    assert all(torch.isfinite(v.float()).all() for v in model.state_dict().values())
