"""The device-resident step seed on the MI355X, kernel level: vc_seed_next against the Python
restatement `seeds.step_seed`, and every `_ds` entry point (the seed read from device memory, plus a site offset)
against its host-seed entry called with the sum: outputs and mask bytes must be the same bits (`torch.equal`), since
both run one kernel body.  The host-seed entry itself is pinned to a numpy restatement of the hash, so the shared body
did not move it.

Shapes: the dropout kernel at n = 1, 63, 64, 65 (around one wave) and 4097 (more than one block, a ragged tail); the
fused sites at B = 1 and 3 and the smallest and largest token counts of tests/test_hctnet_kernels_gpu.py (1 / 8 tokens
over 1 / 81 pixels, sequences of 2 / 9 rows) and tests/test_pixel_kernels_gpu.py (T = 2 and 256), p = 0.1.  Outputs sit
in helpers.Guarded buffers, so a store outside them fails the test.
"""
import numpy as np
import pytest
import torch

from helpers import Guarded
from test_hctnet_kernels_gpu import CT, CT_SHAPES, ENC, ENC_SHAPES, packed, strided, uni

pytestmark = pytest.mark.gpu
DEV = "cuda"
V = 0x2545F4914F6CDD1D >> 2          # the value put into *seed_dev (< 2^62, as vc_seed_next leaves it)
OFFSETS = (0, 1000003 * 3)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vitcnn_amd._lib import lib
    return lib()


def S():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def seed_dev(L):
    """a seed state whose `cur` word holds V (the other words hold values a wrong pointer would show)"""
    st = torch.tensor([111, 222, V, 333], dtype=torch.int64, device=DEV)
    return st, st.data_ptr() + 16


# ---------------------------------------------------------------------------------------------- the seed sequence
@pytest.mark.parametrize("base", [0x0123456789ABCDEF, (1 << 62) - 1 + (1 << 63)])
def test_seed_next_follows_the_python_restatement(L, base):
    from vitcnn_amd import seeds
    st = seeds.SeedState(base, DEV)
    assert st.read() == (base, 0, 0)
    for n in range(1, 6):
        L.vc_seed_next(st.state_ptr, S())
        got = st.read()
        assert got == (base, n, seeds.step_seed(base, n)), (n, got)
        assert got[2] < 1 << 62
        assert int(st.buf[3]) == 0
    assert len({seeds.step_seed(base, n) for n in range(1, 6)}) == 5
    assert L.raw["vc_seed_next"](None, S()) == 1 and L.raw["vc_seed_next"](st.state_ptr + 4, S()) == 1


# ---------------------------------------------------------------------------------------------- vc_dropout_fwd_ds
@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("mode", ["plain", "add", "alias"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_dropout_ds_equals_the_host_seed_entry(L, seed_dev, n, p, mode, off):
    _, cur = seed_dev
    x = uni(n, seed=n).to(DEV)
    add = uni(n, seed=n + 1).to(DEV) if mode == "add" else None
    got = []
    for ds in (False, True):
        mk = Guarded(1, n, dtype=torch.uint8)
        y = Guarded(1, n, init=x) if mode == "alias" else Guarded(1, n)
        xp = y.ptr if mode == "alias" else x.data_ptr()
        ap = add.data_ptr() if add is not None else None
        if ds:
            L.vc_dropout_fwd_ds(n, xp, ap, y.ptr, mk.ptr, p, cur, off, S())
        else:
            L.vc_dropout_fwd(n, xp, ap, y.ptr, mk.ptr, p, V + off, S())
        got.append((y.check(), mk.check()))
    (y0, m0), (y1, m1) = got
    assert torch.equal(m0, m1) and torch.equal(y0, y1)
    assert bool((m0 <= 1).all())
    if n == 4097:
        assert 0 < int(m0.sum()) < n
    assert L.raw["vc_dropout_fwd_ds"](n, x.data_ptr(), None, x.data_ptr(), x.data_ptr(), p, None, off, S()) == 1


# ---------------------------------------------------------------------------------------------- the fused sites
@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C1,C2", [(1, 0), (254, 1)])
def test_sf_embed_ds_equals_the_host_seed_entry(L, seed_dev, C1, C2, B, off):
    _, cur = seed_dev
    D, T, p = 64, C1 + C2 + 1, 0.1
    x1, x2 = uni(B, C1, seed=T).to(DEV), uni(B, max(C2, 1), seed=T + 1).to(DEV)
    w, bias, cls, pos = (uni(*s, seed=T + 2 + i).to(DEV) for i, s in enumerate(((D,), (D,), (D,), (T, D))))
    n = B * T * D
    got = []
    for ds in (False, True):
        X, mask = Guarded(B * T, D), Guarded(1, n, dtype=torch.uint8)
        args = (B, C1, C2, D, x1.data_ptr(), x2.data_ptr() if C2 else None, w.data_ptr(), bias.data_ptr(),
                cls.data_ptr(), pos.data_ptr(), p)
        if ds:
            L.vc_sf_embed_fwd_ds(*args, cur, off, X.ptr, mask.ptr, S())
        else:
            L.vc_sf_embed_fwd(*args, V + off, X.ptr, mask.ptr, S())
        got.append((X.check(), mask.check()))
    assert torch.equal(got[0][1], got[1][1]) and torch.equal(got[0][0], got[1][0])
    assert not got[0][0].isnan().any() and bool((got[0][1] <= 1).all())
    assert L.raw["vc_sf_embed_fwd_ds"](*args, None, off, X.ptr, mask.ptr, S()) == 1


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Lt,HW", [(1, 1), (1, 81), (8, 1), (8, 81)])
def test_tokpool_ds_equals_the_host_seed_entry(L, seed_dev, Lt, HW, B, off):
    _, cur = seed_dev
    ldx, T, p = 68, Lt + 1, 0.1
    Xd = torch.full((B * HW, ldx), float("nan"), device=DEV)
    Xd[:, :64] = uni(B, HW, 64, seed=HW + Lt).reshape(-1, 64).to(DEV)
    wA, wV = (uni(Lt, 64, seed=1) * 0.5).to(DEV), (uni(64, 64, seed=2) * 0.2).to(DEV)
    cls, pos = uni(1, 64, seed=3).to(DEV), uni(T, 64, seed=4).to(DEV)
    got = []
    for ds in (False, True):
        A, U, tok = Guarded(B * Lt, HW), Guarded(B * Lt, 64), Guarded(B * T, 64)
        mask = Guarded(1, B * T * 64, dtype=torch.uint8)
        args = (B, HW, Lt, Xd.data_ptr(), ldx, wA.data_ptr(), wV.data_ptr(), cls.data_ptr(), pos.data_ptr(), p)
        if ds:
            L.vc_hct_tokpool_fwd_ds(*args, cur, off, A.ptr, U.ptr, tok.ptr, mask.ptr, S())
        else:
            L.vc_hct_tokpool_fwd(*args, V + off, A.ptr, U.ptr, tok.ptr, mask.ptr, S())
        got.append([g.check() for g in (A, U, tok, mask)])
    assert all(torch.equal(a, b) for a, b in zip(*got))
    assert not any(t.isnan().any() for t in got[0][:3]) and bool((got[0][3] <= 1).all())
    assert L.raw["vc_hct_tokpool_fwd_ds"](*args, None, off, A.ptr, U.ptr, tok.ptr, mask.ptr, S()) == 1


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [2, 9])
def test_encoder_ds_equals_the_host_seed_entry(L, seed_dev, T, B, off):
    _, cur = seed_dev
    n = B * T * 64
    sx, sy = n + 20, n + 12
    Xd = strided(uni(2, B, T, 64, seed=T + B), sx)
    Wd = [packed(ENC_SHAPES, 100 + 40 * br, (0, 6))[0].to(DEV) for br in (0, 1)]
    assert Wd[0].numel() == ENC
    ps = (0.1,) * 6
    got = []
    for ds in (False, True):
        Y = Guarded(1, sy + n)
        mask = Guarded(1, 2 * B * T * 136, dtype=torch.uint8)
        args = (B, T, Xd.data_ptr(), sx, Wd[0].data_ptr(), Wd[1].data_ptr(), *ps)
        if ds:
            L.vc_hct_encoder_fwd_ds(*args, cur, off, Y.ptr, sy, mask.ptr, S())
        else:
            L.vc_hct_encoder_fwd(*args, V + off, Y.ptr, sy, mask.ptr, S())
        Yg = Y.check()[0]
        got.append((torch.cat((Yg[:n], Yg[sy:sy + n])), mask.check()))
    assert torch.equal(got[0][1], got[1][1]) and torch.equal(got[0][0], got[1][0])
    assert not got[0][0].isnan().any() and bool((got[0][1] <= 1).all())
    assert L.raw["vc_hct_encoder_fwd_ds"](*args, None, off, Y.ptr, sy, mask.ptr, S()) == 1


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [2, 9])
def test_ctattn_ds_equals_the_host_seed_entry(L, seed_dev, T, B, off):
    _, cur = seed_dev
    n = B * T * 64
    sx = n + 20
    Xd = strided(uni(2, B, T, 64, seed=T + B + 7), sx)
    Wd = [packed(CT_SHAPES, 300 + 40 * d, (0,))[0].to(DEV) for d in (0, 1)]
    assert Wd[0].numel() == CT
    ps = (0.1,) * 4
    got = []
    for ds in (False, True):
        out = Guarded(2 * B, 64)
        mask = Guarded(1, 2 * B * (8 * T + 64), dtype=torch.uint8)
        args = (B, T, Xd.data_ptr(), sx, Wd[0].data_ptr(), Wd[1].data_ptr(), *ps)
        if ds:
            L.vc_hct_ctattn_fwd_ds(*args, cur, off, out.ptr, mask.ptr, S())
        else:
            L.vc_hct_ctattn_fwd(*args, V + off, out.ptr, mask.ptr, S())
        got.append((out.check(), mask.check()))
    assert torch.equal(got[0][1], got[1][1]) and torch.equal(got[0][0], got[1][0])
    assert not got[0][0].isnan().any() and bool((got[0][1] <= 1).all())
    assert L.raw["vc_hct_ctattn_fwd_ds"](*args, None, off, out.ptr, mask.ptr, S()) == 1


def test_the_seed_state_is_only_read(L, seed_dev):
    """runs after the _ds tests of this module: none of them wrote a word of the state"""
    st, _ = seed_dev
    assert st.tolist() == [111, 222, V, 333]


# ---------------------------------------------------------------------------------------------- the old entry
def _mix32_keep(seed, n, p):
    """numpy restatement of csrc/s2eft.hip: keep_i = float(mix32(seed, i) >> 8) / 2^24 >= p, all in uint64 / fp32"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) ^ (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        h = ((z ^ (z >> np.uint64(31))) >> np.uint64(32)).astype(np.uint32)
    u = (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return (u >= np.float32(p)).astype(np.uint8)


@pytest.mark.parametrize("seed", [4242, 0x1F2E3D4C5B6A7988])
def test_the_host_seed_entry_did_not_move(L, seed):
    n, p = 4097, 0.1
    want = _mix32_keep(seed, n, p)
    x = uni(n, seed=5).to(DEV)
    y, mk = Guarded(1, n), Guarded(1, n, dtype=torch.uint8)
    L.vc_dropout_fwd(n, x.data_ptr(), None, y.ptr, mk.ptr, p, seed, S())
    got = mk.check()[0].numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    keep = torch.from_numpy(want).bool()
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    ref = torch.where(keep, x.cpu() * float(scale), torch.zeros(n))
    assert torch.equal(y.check()[0], ref)
