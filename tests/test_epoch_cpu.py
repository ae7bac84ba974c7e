"""The per-epoch reshuffle and the device augmentation draws, the host side (no GPU): `window.epoch_order` and
`window.device_decisions` -- the numpy restatements the kernels vc_epoch_shuffle / vc_aug_draw are held to in
test_epoch_kernels_gpu.py -- against their contract (include/vitcnn.h), and PatchBatcher's refusals."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


def mix64(z):
    """the splitmix64 finaliser in Python integers (independent of the package's array form)"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def keys_ref(N, seed, epoch, key_bits):
    from vitcnn_amd.window import SHUFFLE_DOMAIN
    base = mix64(((seed ^ SHUFFLE_DOMAIN) + epoch) & M64)
    return np.array([mix64((base + j) & M64) >> (64 - key_bits) for j in range(N)], dtype=np.uint64)


def test_constants_are_the_headers():
    from vitcnn_amd import window as W
    text = open(os.path.join(REPO, "include", "vitcnn.h")).read()
    assert int(re.search(r"#define VC_SHUFFLE_DOMAIN (0x[0-9A-Fa-f]+)ull", text).group(1), 16) == W.SHUFFLE_DOMAIN
    assert re.search(r"#define VC_SHUFFLE_MAX \(1 << (\d+)\)", text).group(1) == "17" and W.SHUFFLE_MAX == 1 << 17
    for name, want in (("FLIP", W.AUG_FLIP), ("RADIATION", W.AUG_RADIATION), ("MIXTURE", W.AUG_MIXTURE)):
        assert int(re.search(rf"#define VC_AUG_{name} (\d+)", text).group(1)) == want


@pytest.mark.parametrize("N", [1, 2, 10, 1000])
def test_epoch_order_is_a_deterministic_permutation(N):
    from vitcnn_amd.window import epoch_order
    a = epoch_order(N, 7, 3)
    assert a.dtype == np.int32 and a.shape == (N,)
    assert np.array_equal(np.sort(a), np.arange(N))
    assert np.array_equal(a, epoch_order(N, 7, 3))


def test_epoch_order_differs_between_epochs_and_seeds():
    from vitcnn_amd.window import epoch_order
    a = epoch_order(1000, 7, 0)
    assert not np.array_equal(a, epoch_order(1000, 7, 1))
    assert not np.array_equal(a, epoch_order(1000, 8, 0))
    assert not np.array_equal(a, np.arange(1000))
    # epoch e of seed s is not epoch e + 1 of seed s - 1 and the like: the base is hashed, not added to the index
    assert not np.array_equal(epoch_order(1000, 7, 1), epoch_order(1000, 8, 0))


@pytest.mark.parametrize("key_bits", [64, 8, 1])
def test_epoch_order_is_the_stable_argsort_of_the_keys(key_bits):
    """at 8 bits 1000 elements share 256 keys, at 1 bit two: ties keep the smaller index first"""
    from vitcnn_amd.window import epoch_keys, epoch_order
    N = 1000
    keys = keys_ref(N, 12345, 5, key_bits)
    assert np.array_equal(epoch_keys(N, 12345, 5, key_bits), keys)
    if key_bits < 64:
        assert len(np.unique(keys)) <= 1 << key_bits < N
    else:
        assert len(np.unique(keys)) == N
    got = epoch_order(N, 12345, 5, key_bits=key_bits)
    assert np.array_equal(got, np.argsort(keys, kind="stable"))
    # and by the definition: perm[r] = j for the j with r pairs (key, index) below its own
    pairs = sorted((int(k), j) for j, k in enumerate(keys))
    assert got.tolist() == [j for _, j in pairs]


def test_no_tie_at_64_bits_at_the_bound():
    from vitcnn_amd.window import SHUFFLE_MAX, epoch_keys
    assert len(np.unique(epoch_keys(SHUFFLE_MAX, 0, 0))) == SHUFFLE_MAX
    assert SHUFFLE_MAX - len(np.unique(epoch_keys(SHUFFLE_MAX, 0, 0, 8))) == SHUFFLE_MAX - 256


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("N", [1, 2, 10, 1000])
def test_epoch_order_shards(N, world):
    from vitcnn_amd.window import epoch_order
    perm = epoch_order(N, 3, 2)
    per = -(-N // world)
    shards = [epoch_order(N, 3, 2, rank, world) for rank in range(world)]
    for rank, s in enumerate(shards):
        assert s.shape == (per,)                                   # equal length on every rank
        assert np.array_equal(s, np.resize(perm, per * world)[rank::world])
    assert set(np.concatenate(shards).tolist()) == set(range(N))   # their union is everything
    if N % world == 0:
        assert len(set(np.concatenate(shards).tolist())) == per * world    # and without padding they are disjoint


def test_epoch_order_refusals():
    from vitcnn_amd.window import SHUFFLE_MAX, epoch_order
    for bad in (dict(N=0), dict(N=SHUFFLE_MAX + 1), dict(rank=2, world=2), dict(rank=-1), dict(world=0),
                dict(key_bits=0), dict(key_bits=65)):
        kw = dict(N=10, seed=0, epoch=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            epoch_order(**kw)


# ---------------------------------------------------------------------------------------------- device_decisions
N_DRAWS = 200_000


def _events(codes, rad, mix):
    """event name -> (boolean array, the reference's probability): datasets.py:559-568, :511-526"""
    rot = codes >> 2
    ev = {
        "horizontal flip": (codes & 1 != 0, 0.25),
        "vertical flip": (codes & 2 != 0, 0.25),
        "rotation": (rot != 0, 0.25),
        "radiation": (rad != 0, 0.1),
        "mixture": (mix[:, 0] > 0, 0.2),
        "radiation and mixture": ((rad != 0) & (mix[:, 0] > 0), 0.02),
        # code 0 arises in the flip branch with both flips clear (1/8) and when neither branch is taken (1/4)
        "no transform": (codes == 0, 0.375),
    }
    for k in (1, 2, 3):
        ev[f"rotation k={k}"] = (rot == k, 1.0 / 12.0)
    return ev


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_device_decisions_frequencies(seed):
    """every event of the reference's tree within 4 binomial standard deviations of its probability over 200,000
    consecutive ids (evaluated when this test was written: all within 1.9).  The flip branch itself (0.5) is read
    from the uniforms' definition, since the code does not tell a flip branch that cleared both flips from no branch."""
    from vitcnn_amd.window import device_decisions
    codes, rad, mix = device_decisions(seed, 0, N_DRAWS, True, True, True)
    assert codes.dtype == np.uint8 and rad.dtype == np.float32 and mix.dtype == np.float32
    assert codes.shape == (N_DRAWS,) and rad.shape == (N_DRAWS,) and mix.shape == (N_DRAWS, 2)
    ev = _events(codes, rad, mix)
    # the flip branch: u0 > 0.5, from the definition of the draws
    u0 = np.array([mix64(_dkey(seed, g)) >> 40 for g in range(N_DRAWS)]) * 2.0 ** -24
    ev["flip branch"] = (u0 > 0.5, 0.5)
    assert np.array_equal((u0 > 0.5) & (codes != 0), codes & 3 != 0)    # flips come from the flip branch only
    worst = 0.0
    for name, (hit, p) in ev.items():
        z = (hit.mean() - p) / np.sqrt(p * (1 - p) / hit.size)
        print(f"seed {seed}: {name}: {hit.mean():.5f} against {p:.5f}, z = {z:+.2f}")
        worst = max(worst, abs(z))
        assert abs(z) < 4.0, (name, float(hit.mean()), p, float(z))
    print(f"seed {seed}: worst |z| = {worst:.2f}")
    # codes are valid gather codes: flip bits and rotation never together
    assert not np.any((codes & 3 != 0) & (codes >> 2 != 0)) and codes.max() <= 12
    r = rad[rad != 0]
    assert r.min() >= np.float32(0.9) and r.max() <= np.float32(1.1) and abs(r.mean() - 1.0) < 0.002
    m = mix[mix[:, 0] > 0]
    assert m.min() >= np.float32(0.01) and m.max() <= np.float32(1.0)
    assert np.all((mix[:, 0] > 0) == (mix[:, 1] > 0))


def _dkey(seed, gid):
    return mix64(seed ^ mix64(((gid << 2) | 3) & M64))


def test_device_decisions_follow_the_definition():
    """the vectorised restatement against the tree written out in Python integers and one float64 -> float32 rounding"""
    from vitcnn_amd.window import device_decisions
    f32 = np.float32
    for seed, gid0 in ((5, 0), (12345, 1 << 40)):
        codes, rad, mix = device_decisions(seed, gid0, 400, True, True, True)
        for i in range(400):
            dk = _dkey(seed, gid0 + i)
            u = [f32((mix64((dk + e) & M64) >> 40) * 2.0 ** -24) for e in range(10)]
            code = 0
            if u[0] > 0.5:
                code = int(u[1] > 0.5) | int(u[2] > 0.5) << 1
            elif u[3] > 0.5:
                code = (1 + min(2, int(f32(3.0) * u[4]))) << 2
            a = f32(float(f32(0.2)) * float(u[6]) + float(f32(0.9))) if u[5] < f32(0.1) else f32(0)
            a1 = a2 = f32(0)
            if u[7] < f32(0.2):
                a1 = f32(float(f32(0.99)) * float(u[8]) + float(f32(0.01)))
                a2 = f32(float(f32(0.99)) * float(u[9]) + float(f32(0.01)))
            assert (codes[i], rad[i], mix[i, 0], mix[i, 1]) == (code, a, a1, a2), (seed, gid0, i)


def test_device_decisions_consecutive_batches_are_one_stream():
    from vitcnn_amd.window import device_decisions
    whole = device_decisions(9, 100, 64, True, True, True)
    parts = [device_decisions(9, 100 + o, n, True, True, True) for o, n in ((0, 30), (30, 34))]
    for w, a, b in zip(whole, *parts):
        assert np.array_equal(w, np.concatenate([a, b]))


@pytest.mark.parametrize("flip,radiation,mixture", [(f, r, m) for f in (0, 1) for r in (0, 1) for m in (0, 1)])
def test_device_decisions_switched_off_gives_zeros(flip, radiation, mixture):
    from vitcnn_amd.window import device_decisions
    full = device_decisions(3, 0, 5000, True, True, True)
    codes, rad, mix = device_decisions(3, 0, 5000, flip, radiation, mixture)
    for on, got, want in ((flip, codes, full[0]), (radiation, rad, full[1]), (mixture, mix, full[2])):
        assert got.dtype == want.dtype and got.shape == want.shape
        # an enabled augmentation does not depend on the others; a disabled one is all zeros
        assert np.array_equal(got, want) if on else not got.any()
    assert device_decisions(3, 0, 0, True, True, True)[2].shape == (0, 2)


# ---------------------------------------------------------------------------------------------- PatchBatcher
def _scene(W=12, H=10):
    rng = np.random.default_rng(0)
    return (rng.random((W, H, 3), dtype=np.float32), rng.random((W, H, 1), dtype=np.float32),
            rng.integers(0, 4, size=(W, H)))


def test_unknown_shuffle_or_draws_is_refused():
    """before anything touches a device: these run without one"""
    from vitcnn_amd.window import PatchBatcher
    img1, img2, gt = _scene()
    for kw in (dict(shuffle="batch"), dict(shuffle=True), dict(shuffle="Epoch"), dict(draws="gpu"), dict(draws=None)):
        with pytest.raises(ValueError, match="unknown (shuffle|draws)"):
            PatchBatcher(img1, img2, gt, 5, device="cuda", **kw)


def test_oversized_list_is_refused_with_epoch_shuffle():
    from vitcnn_amd.window import SHUFFLE_MAX, PatchBatcher
    W, H = 364, 364                                   # 364 * 364 = 132,496 labelled pixels > 131,072
    img1, img2, gt = np.zeros((W, H, 1), np.float32), np.zeros((W, H, 1), np.float32), np.ones((W, H), np.int64)
    assert W * H > SHUFFLE_MAX
    with pytest.raises(ValueError, match="shuffle='epoch'"):
        PatchBatcher(img1, img2, gt, 1, device="cpu", border="symmetric", shuffle="epoch")
    PatchBatcher(img1, img2, gt, 1, device="cpu", border="symmetric")           # the default takes any length
    with pytest.raises(ValueError, match="shuffle='epoch'"):                    # and an empty list has no order
        PatchBatcher(img1, img2, np.zeros((W, H), np.int64), 1, device="cpu", shuffle="epoch")


def test_default_cpu_batcher_is_unaffected():
    from vitcnn_amd.window import PatchBatcher
    img1, img2, gt = _scene()
    a = PatchBatcher(img1, img2, gt, 5, batch_size=4, device="cpu", seed=3)
    b = PatchBatcher(img1, img2, gt, 5, batch_size=4, device="cpu", seed=3, shuffle=None, draws="host")
    assert a.shuffle is None and a.draws == "host"
    assert np.array_equal(a.centers, b.centers) and len(a) == len(b) == -(-len(a.centers) // 4)
    assert np.array_equal(a.corners.numpy(), (a.centers - 2).astype(np.int32))
    # the construction-time order is RandomState(seed).shuffle of the row-major labelled pixels
    xs, ys = np.nonzero(gt)
    keep = (xs > 2) & (xs < 10) & (ys > 2) & (ys < 8)
    idx = np.stack([xs[keep], ys[keep]], axis=1)
    np.random.RandomState(3).shuffle(idx)
    assert np.array_equal(a.centers, idx)
    assert np.array_equal(a.labels.numpy(), gt[idx[:, 0], idx[:, 1]])


def test_cpu_batcher_with_epoch_shuffle_holds_epoch_0():
    """construction needs no device: corners / labels / centers are epoch 0's shard of the whole list"""
    from vitcnn_amd.window import PatchBatcher, epoch_order
    img1, img2, gt = _scene()
    base = PatchBatcher(img1, img2, gt, 5, batch_size=4, device="cpu", seed=3)
    N = len(base.centers)
    for rank in (0, 1):
        pb = PatchBatcher(img1, img2, gt, 5, batch_size=4, device="cpu", seed=3, rank=rank, world=2, shuffle="epoch")
        order = epoch_order(N, 3, 0, rank, 2)
        assert np.array_equal(pb.centers, base.centers[order])
        assert np.array_equal(pb.corners.numpy(), (base.centers[order] - 2).astype(np.int32))
        assert np.array_equal(pb.labels.numpy(), base.labels.numpy()[order])
        assert len(pb) == -(-len(order) // 4)
        pb.epoch = 4                                   # `centers` follows the epoch the lists hold
        assert np.array_equal(pb.centers, base.centers[epoch_order(N, 3, 4, rank, 2)])
