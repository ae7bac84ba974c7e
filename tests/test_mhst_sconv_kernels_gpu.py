"""vc_mhst_conv1_fwd / _wgrad and vc_mhst_sconv_fwd / _dgrad / _wgrad (csrc/mhst_sconv.hip) against float64 F.conv3d and
autograd (the four spectral convolutions concatenated on the channel axis), in test_mhst_pconv_kernels_gpu's harness:
poisoned inputs (row padding and the lead of every weight and bias hold NaN), guarded or sentinel-filled outputs checked
outside the written columns, a guarded workspace of exactly the queried size, and a second call that must give the same
bits.  Bound: 1e-4 of the tensor's largest magnitude, the kernel classes' bound (DESIGN.md sections 16 and 22).

The shapes are the smallest at which the kernels can still go wrong.  conv1: l1 = 1, 2 have one output depth whose taps
mostly lie outside; 10 .. 13 step D1 from 4 to 5 across the three residues of the stride, which is also the forward's
chunk (VC_MHST_CONV1_CHUNK = 4 output depths per block) and the chunk plus one; 144 is the model's.  The weight gradient
launches min(VC_MHST_CONV1_WAVES = 1024, B D1) waves: l1 = 1030 at B = 3 has 1032 planes, every other case fewer.
sconv: D = 1 has centre taps only; up to D = 5 the 11-tap convolution never has all its taps inside; 6 and 11 are the
first depths with 6 and all 11 inside somewhere; a block owns VC_MHST_SCONV_CHUNK = 4 depths (3, 5: a chunk not full);
the weight gradient launches min(VC_MHST_SCONV_BLOCKS = 256, B ceil(D / 4)) blocks: D = 345 at B = 3 has 261 items."""
import re

import pytest
import torch
import torch.nn.functional as F

from helpers import GUARD, SENTINEL, Guarded, Poisoned, within

pytestmark = pytest.mark.gpu
BOUND = 1e-4
CONV1_CHUNK, CONV1_WAVES, SCONV_CHUNK, SCONV_BLOCKS = 4, 1024, 4, 256
TAPS = (1, 3, 5, 11)


def L():
    from vitcnn_amd._lib import lib
    return lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def rnd(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1


def close(kernel, shape, got, want):
    want = want.reshape(got.shape)
    within(kernel, shape, float((got.double() - want).abs().max()), BOUND * max(float(want.abs().max()), 1e-30))


def rows(t):
    """[B, C, D, 8, 8] -> channels-last rows (b, d, h, w) of C columns"""
    return t.detach().permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])


def test_the_constants_are_the_header_s():
    from vitcnn_amd._lib import header_path
    text = open(header_path()).read()
    for name, v in (("CONV1_CHUNK", CONV1_CHUNK), ("CONV1_WAVES", CONV1_WAVES), ("SCONV_CHUNK", SCONV_CHUNK),
                    ("SCONV_BLOCKS", SCONV_BLOCKS)):
        assert int(re.search(rf"#define VC_MHST_{name} (\d+)", text).group(1)) == v, name


def out_rows(call, M, ld):
    """a 16-column output inside rows of ld floats: everything else in the buffer must stay untouched"""
    flat = torch.full((M * ld + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    call(flat.data_ptr())
    torch.cuda.synchronize()
    flat = flat.cpu()
    got = flat.as_strided((M, 16), (ld, 1), 0).clone()
    flat.as_strided((M, 16), (ld, 1), 0).fill_(SENTINEL)
    assert bool((flat == SENTINEL).all()), "store outside the 16 columns"
    return got


# name: (B, l1, ldy)
CONV1 = {f"l1={l1}": (1 + i % 3, l1, 16) for i, l1 in enumerate((1, 2, 4, 10, 11, 12, 13, 30))}
CONV1.update({
    "l1=144 (D1 = 48)": (1, 144, 16),
    "l1=12 rows of 20 floats (D1 = the chunk)": (2, 12, 20),
    "l1=13 rows of 20 floats (D1 = the chunk + 1)": (3, 13, 20),
    "l1=1030 B=3 (1032 planes, 1024 waves)": (3, 1030, 16),
})


@pytest.mark.parametrize("name", list(CONV1))
def test_conv1(name):
    B, l1, ldy = CONV1[name]
    D1 = (l1 + 2) // 3
    if "chunk" in name:
        assert D1 == CONV1_CHUNK + ("+ 1" in name)
    assert (B * D1 > CONV1_WAVES) == ("1032" in name)
    g = torch.Generator().manual_seed(2)
    x = rnd(g, B, 1, l1, 8, 8)
    w = rnd(g, 16, 1, 11, 3, 3).requires_grad_(True)
    bias = rnd(g, 16).requires_grad_(True)
    y = F.conv3d(x, w, bias, stride=(3, 1, 1), padding=(5, 1, 1))
    assert y.shape[2] == D1
    dy = rnd(g, *y.shape)
    y.backward(dy)
    M = B * D1 * 64
    xd = Poisoned(x.reshape(1, -1).float())
    wd = Poisoned(w.detach().reshape(1, -1).float(), lead=1)
    bd = Poisoned(bias.detach().reshape(1, -1).float(), lead=3)
    dyd = Poisoned(rows(dy).float(), ld=ldy)
    n = L().vc_mhst_conv1_ws_floats(B, l1)
    ws = Guarded(1, n)

    def fwd(b):
        got = out_rows(lambda p: L().vc_mhst_conv1_fwd(B, l1, xd.ptr, wd.ptr, b, p, ldy, ws.ptr, n, stream()), M, ldy)
        ws.check()
        return got

    got = fwd(bd.ptr)
    close("vc_mhst_conv1_fwd", name, got, rows(y))
    assert torch.equal(fwd(bd.ptr), got)      # a second run: the same bits
    close("vc_mhst_conv1_fwd no bias", name, fwd(None), rows(y) - bias.detach())

    dwg, dbg = Guarded(1, w.numel()), Guarded(1, 16)
    L().vc_mhst_conv1_wgrad(B, l1, xd.ptr, dyd.ptr, ldy, dwg.ptr, dbg.ptr, ws.ptr, n, stream())
    got = dwg.check()
    ws.check()
    close("vc_mhst_conv1_wgrad", name, got, w.grad)
    close("vc_mhst_conv1_wgrad bias", name, dbg.check(), bias.grad)
    dwg = Guarded(1, w.numel())
    L().vc_mhst_conv1_wgrad(B, l1, xd.ptr, dyd.ptr, ldy, dwg.ptr, None, ws.ptr, n, stream())
    assert torch.equal(dwg.check(), got)      # a second run, without db: the same bits
    ws.check()


# name: (B, D, ldx, ldy)
SCONV = {f"D={D}": (1 + i % 3, D, 16, 16) for i, D in enumerate((1, 2, 3, 5, 6, 10, 11, 48))}
SCONV.update({
    "D=5 x rows of 20 floats": (2, 5, 20, 16),
    "D=6 y rows of 20 floats": (3, 6, 16, 20),
    "D=11 both rows of 20 floats": (1, 11, 20, 20),
    "D=345 B=3 (261 items, 256 blocks)": (3, 345, 16, 16),
})


@pytest.mark.parametrize("name", list(SCONV))
def test_sconv(name):
    B, D, ldx, ldy = SCONV[name]
    assert (B * ((D + SCONV_CHUNK - 1) // SCONV_CHUNK) > SCONV_BLOCKS) == ("261" in name)
    g = torch.Generator().manual_seed(3)
    x = rnd(g, B, 16, D, 8, 8).requires_grad_(True)
    ws_ = [rnd(g, 4, 16, k, 1, 1).requires_grad_(True) for k in TAPS]
    bs_ = [rnd(g, 4).requires_grad_(True) for _ in TAPS]
    y = torch.cat([F.conv3d(x, w, b, padding=(k // 2, 0, 0)) for w, b, k in zip(ws_, bs_, TAPS)], dim=1)
    dy = rnd(g, *y.shape)
    y.backward(dy)
    M = B * D * 64
    xd = Poisoned(rows(x).float(), ld=ldx)
    dyd = Poisoned(rows(dy).float(), ld=ldy)
    wd = [Poisoned(w.detach().reshape(1, -1).float(), lead=1 + i % 3) for i, w in enumerate(ws_)]
    bd = [Poisoned(b.detach().reshape(1, -1).float(), lead=3 - i % 3) for i, b in enumerate(bs_)]
    wp, bp = [t.ptr for t in wd], [t.ptr for t in bd]
    n = L().vc_mhst_sconv_ws_floats(B, D)
    ws = Guarded(1, n)

    def fwd(b):
        got = out_rows(lambda p: L().vc_mhst_sconv_fwd(B, D, xd.ptr, ldx, *wp, *b, p, ldy, ws.ptr, n, stream()), M, ldy)
        ws.check()
        return got

    got = fwd(bp)
    close("vc_mhst_sconv_fwd", name, got, rows(y))
    assert torch.equal(fwd(bp), got)          # a second run: the same bits
    close("vc_mhst_sconv_fwd no biases", name, fwd([None] * 4), rows(y) - torch.cat([b.detach() for b in bs_]))

    init = rnd(g, M, 16).float()
    for beta in (0.0, 1.0):
        dxg = Guarded(M, 16, ld=ldx, init=init if beta else None)
        L().vc_mhst_sconv_dgrad(B, D, dyd.ptr, ldy, *wp, dxg.ptr, ldx, beta, ws.ptr, n, stream())
        got = dxg.check()
        close("vc_mhst_sconv_dgrad", f"{name} beta {beta}", got, rows(x.grad) + beta * init.double())
        ws.check()
        dxg = Guarded(M, 16, ld=ldx, init=init if beta else None)
        L().vc_mhst_sconv_dgrad(B, D, dyd.ptr, ldy, *wp, dxg.ptr, ldx, beta, ws.ptr, n, stream())
        assert torch.equal(dxg.check(), got)  # a second run: the same bits

    def wgrad(with_db):
        dwg = [Guarded(1, w.numel()) for w in ws_]
        dbg = [Guarded(1, 4) for _ in TAPS]
        L().vc_mhst_sconv_wgrad(B, D, xd.ptr, ldx, dyd.ptr, ldy, *(t.ptr for t in dwg),
                                *((t.ptr for t in dbg) if with_db else [None] * 4), ws.ptr, n, stream())
        ws.check()
        return [t.check() for t in dwg], [t.check() for t in dbg]

    dws, dbs = wgrad(True)
    for i, k in enumerate(TAPS):
        close(f"vc_mhst_sconv_wgrad k={k}", name, dws[i], ws_[i].grad)
        close(f"vc_mhst_sconv_wgrad bias k={k}", name, dbs[i], bs_[i].grad)
    again, untouched = wgrad(False)
    assert all(torch.equal(a, b) for a, b in zip(again, dws))   # a second run, without db: the same bits
    assert all(bool(torch.isnan(t).all()) for t in untouched)   # and the bias gradients are not written
