"""vc_epoch_shuffle and vc_aug_draw against their numpy restatements (`window.epoch_order`, `window.device_decisions`):
array equality at sizes around the block and LDS-tile edges, every shard, forced ties, outputs inside poisoned guard
buffers, and the refusals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 1024
POISON = -7777
SEED = 0x1234_5678_9ABC_DEF1 & ((1 << 63) - 1)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _guarded(n, dtype, poison=POISON):
    """(whole buffer, the n-element window in its middle): everything holds `poison`"""
    buf = torch.full((GUARD + n + GUARD,), poison, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, n, poison=POISON):
    b = buf.cpu()
    return bool((b[:GUARD] == poison).all()) and bool((b[GUARD + n:] == poison).all())


def _lists(N):
    rng = np.random.default_rng(N)
    corners = rng.integers(-4, 2000, size=(N, 2)).astype(np.int32)
    labels = rng.integers(0, 1 << 40, size=N).astype(np.int64)
    return corners, labels


def _shuffle(L, N, epoch, rank, world, key_bits, cd, ld, with_order, seed=SEED):
    """one launch into guarded outputs -> (corners_out, labels_out, order_out or None) as numpy, guards checked"""
    per = -(-N // world)
    cbuf, cout = _guarded(2 * per, torch.int32)
    lbuf, lout = _guarded(per, torch.int64)
    obuf, oout = _guarded(per, torch.int32)
    L.vc_epoch_shuffle(N, seed, epoch, rank, world, key_bits, cd.data_ptr(), ld.data_ptr(), cout.data_ptr(),
                       lout.data_ptr(), oout.data_ptr() if with_order else None,
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _intact(cbuf, 2 * per) and _intact(lbuf, per) and _intact(obuf, per)
    if not with_order:
        assert bool((oout == POISON).all())
    return cout.cpu().numpy().reshape(per, 2), lout.cpu().numpy(), oout.cpu().numpy() if with_order else None


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 1000, 4099])
def test_epoch_shuffle_is_epoch_order(N):
    """1, 2: degenerate lists (world 3 > N wraps a shard more than once); 63 / 64 / 65: a wave; 257: a second block
    with one live thread; 1000: below one 1024-key LDS tile; 4099: five tiles, the last with 3 keys, 17 blocks"""
    _need_gpu()
    from vitcnn_amd._lib import lib
    from vitcnn_amd.window import epoch_order
    L = lib()
    corners, labels = _lists(N)
    cd, ld = torch.from_numpy(corners).to(DEV), torch.from_numpy(labels).to(DEV)
    for key_bits in (64, 8):
        for epoch in (0, 5):
            for world in (1, 2, 3):
                for rank in range(world):
                    want = epoch_order(N, SEED, epoch, rank, world, key_bits)
                    for with_order in (True, False):
                        c, l, o = _shuffle(L, N, epoch, rank, world, key_bits, cd, ld, with_order)
                        where = (N, key_bits, epoch, rank, world, with_order)
                        if with_order:
                            assert o.dtype == np.int32 and np.array_equal(o, want), where
                        assert np.array_equal(c, corners[want]), where
                        assert np.array_equal(l, labels[want]), where
    assert np.array_equal(cd.cpu().numpy(), corners) and np.array_equal(ld.cpu().numpy(), labels)   # inputs untouched


def test_epoch_shuffle_at_the_bound():
    """N = VC_SHUFFLE_MAX = 131,072: 512 blocks x 128 tiles; at 8 bits all but 256 keys are tied"""
    _need_gpu()
    from vitcnn_amd._lib import lib
    from vitcnn_amd.window import SHUFFLE_MAX, epoch_order
    N = SHUFFLE_MAX
    corners, labels = _lists(N)
    cd, ld = torch.from_numpy(corners).to(DEV), torch.from_numpy(labels).to(DEV)
    for key_bits, rank, world in ((64, 1, 3), (8, 0, 1)):
        want = epoch_order(N, SEED, 5, rank, world, key_bits)
        c, l, o = _shuffle(lib(), N, 5, rank, world, key_bits, cd, ld, True)
        assert np.array_equal(o, want) and np.array_equal(c, corners[want]) and np.array_equal(l, labels[want])


def test_epoch_shuffle_refusals_write_nothing():
    _need_gpu()
    from vitcnn_amd._lib import lib
    from vitcnn_amd.window import SHUFFLE_MAX
    raw = lib().raw["vc_epoch_shuffle"]
    N = 100
    corners, labels = _lists(N)
    cd, ld = torch.from_numpy(corners).to(DEV), torch.from_numpy(labels).to(DEV)
    cbuf, cout = _guarded(2 * N, torch.int32)
    lbuf, lout = _guarded(N, torch.int64)
    obuf, oout = _guarded(N, torch.int32)
    s = torch.cuda.current_stream().cuda_stream
    ok = dict(N=N, seed=SEED, epoch=0, rank=0, world=1, key_bits=64, corners=cd.data_ptr(), labels=ld.data_ptr(),
              corners_out=cout.data_ptr(), labels_out=lout.data_ptr(), order_out=oout.data_ptr())
    bad = [dict(corners=None), dict(labels=None), dict(corners_out=None), dict(labels_out=None), dict(N=0), dict(N=-1),
           dict(N=SHUFFLE_MAX + 1), dict(rank=-1), dict(rank=1), dict(rank=2, world=2), dict(world=0),
           dict(key_bits=0), dict(key_bits=65), dict(key_bits=-1)]
    for b in bad:
        a = dict(ok)
        a.update(b)
        assert raw(a["N"], a["seed"], a["epoch"], a["rank"], a["world"], a["key_bits"], a["corners"], a["labels"],
                   a["corners_out"], a["labels_out"], a["order_out"], s) == 1, b
    torch.cuda.synchronize()
    for buf in (cbuf, lbuf, obuf):
        assert bool((buf == POISON).all())
    assert raw(*[ok[k] for k in ("N", "seed", "epoch", "rank", "world", "key_bits", "corners", "labels", "corners_out",
                                 "labels_out", "order_out")], s) == 0       # the accepted call differs only in those


FLAG_SETS = [(f, r, m) for f in (0, 1) for r in (0, 1) for m in (0, 1)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_aug_draw_is_device_decisions(n):
    _need_gpu()
    from vitcnn_amd._lib import lib
    from vitcnn_amd.window import AUG_FLIP, AUG_MIXTURE, AUG_RADIATION, device_decisions
    L = lib()
    s = torch.cuda.current_stream().cuda_stream
    for gid0 in (0, 1 << 40):
        for flip, radiation, mixture in FLAG_SETS:
            flags = flip * AUG_FLIP | radiation * AUG_RADIATION | mixture * AUG_MIXTURE
            xbuf, xf = _guarded(n, torch.uint8, 0xA5)
            rbuf, rad = _guarded(n, torch.float32)
            mbuf, mix = _guarded(2 * n, torch.float32)
            L.vc_aug_draw(n, flags, SEED, gid0, xf.data_ptr(), rad.data_ptr(), mix.data_ptr(), s)
            torch.cuda.synchronize()
            assert _intact(xbuf, n, 0xA5) and _intact(rbuf, n) and _intact(mbuf, 2 * n)
            codes, alpha, a12 = device_decisions(SEED, gid0, n, flip, radiation, mixture)
            where = (n, gid0, flags)
            assert np.array_equal(xf.cpu().numpy(), codes), where
            # bit equality: compare the float32 words
            assert np.array_equal(rad.cpu().numpy().view(np.uint32), alpha.view(np.uint32)), where
            assert np.array_equal(mix.cpu().numpy().view(np.uint32), a12.reshape(-1).view(np.uint32)), where
            if n == 1000 and flags == 7:     # the case is not vacuous: every branch of the tree occurs
                assert set(codes.tolist()) == {0, 1, 2, 3, 4, 8, 12} and alpha.any() and a12.any()


def test_aug_draw_refusals_write_nothing():
    _need_gpu()
    from vitcnn_amd._lib import lib
    raw = lib().raw["vc_aug_draw"]
    n = 10
    xbuf, xf = _guarded(n, torch.uint8, 0xA5)
    rbuf, rad = _guarded(n, torch.float32)
    mbuf, mix = _guarded(2 * n, torch.float32)
    s = torch.cuda.current_stream().cuda_stream
    x, r, m = xf.data_ptr(), rad.data_ptr(), mix.data_ptr()
    assert raw(-1, 7, SEED, 0, x, r, m, s) == 1
    assert raw(n, 8, SEED, 0, x, r, m, s) == 1
    assert raw(n, -1, SEED, 0, x, r, m, s) == 1
    assert raw(n, 7, SEED, 0, None, r, m, s) == 1
    assert raw(n, 7, SEED, 0, x, None, m, s) == 1
    assert raw(n, 7, SEED, 0, x, r, None, s) == 1
    assert raw(0, 7, SEED, 0, None, None, None, s) == 0            # nothing to draw is not an error
    torch.cuda.synchronize()
    assert bool((xbuf == 0xA5).all()) and bool((rbuf == POISON).all()) and bool((mbuf == POISON).all())
    assert raw(n, 7, SEED, 0, x, r, m, s) == 0
