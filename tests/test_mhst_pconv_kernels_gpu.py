"""vc_mhst_pconv_fwd / _dgrad / _wgrad (csrc/mhst_pconv.hip) against float64 F.conv3d and autograd, in test_conv_family's
harness: poisoned inputs (row padding, the neighbouring columns of x's rows and of dy's rows, the lead of w and bias hold
NaN), sentinel-filled outputs checked outside the part's columns, a guarded workspace of exactly vc_mhst_pconv_ws_floats
floats, and a second call that must give the same bits.  Bound: 1e-4 of the tensor's largest magnitude, the kernel
classes' bound (DESIGN.md sections 16 and 22).

The shapes are the smallest at which the family can still go wrong.  The forward stages VC_MHST_PCONV_CHUNK = 4 depths
per block (2 at 32 channels per group): D = 1, 3 stay inside one chunk and write y directly; D = 10, 13, 48 take the
partial-sum path, 13 and 10 with a last chunk that is not full.  At G = 8 a group has 2 channels, fewer than one MFMA's k
(D = 1: K per tap = 2; D = 3: 6, no multiple of 4).  B = 1, 3, 5 leave the second sample of a forward block empty."""
import pytest
import torch
import torch.nn.functional as F

from helpers import GUARD, SENTINEL, Guarded, Poisoned, within

pytestmark = pytest.mark.gpu
BOUND = 1e-4
CHUNK = 4   # VC_MHST_PCONV_CHUNK

HSI = {"k3 g1": (1, 3, 0), "k5 g2": (2, 5, 16), "k7 g4": (4, 7, 32), "k9 g8": (8, 9, 48)}   # G, KS, its columns of 64

# name: (B, D, C, O, G, KS, ldx, ycol, ldy)
CASES = {}
for _i, (_k, (_g, _ks, _col)) in enumerate(HSI.items()):
    for _j, _d in enumerate((1, 3, 10)):
        CASES[f"hsi {_k} D={_d}"] = (1 + (_i + _j) % 3, _d, 16, 16, _g, _ks, 16, _col, 64)
CASES.update({
    "hsi k3 g1 D=48": (1, 48, 16, 16, 1, 3, 16, 0, 64),
    "hsi k9 g8 D=48": (1, 48, 16, 16, 8, 9, 16, 48, 64),
    "hsi k5 g2 D=13 (3 chunks of 4 and one depth)": (2, 13, 16, 16, 2, 5, 16, 16, 64),
    "hsi k7 g4 D=3 B=5": (5, 3, 16, 16, 4, 7, 16, 32, 64),
    "hsi k3 g1 D=3 B=9 (3 sample splits in the weight gradient)": (9, 3, 16, 16, 1, 3, 16, 0, 64),
    "hsi k5 g2 D=3 rows of 20 floats": (2, 3, 16, 16, 2, 5, 20, 16, 64),
    "lidar 32 -> 16 k3": (2, 1, 32, 16, 1, 3, 32, 0, 64),
    "lidar 32 -> 16 k9": (3, 1, 32, 16, 1, 9, 32, 48, 64),
    "classifier k5 g2": (2, 1, 64, 16, 2, 5, 64, 16, 32),
})


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


def test_the_chunk_is_the_header_s():
    import re
    from vitcnn_amd._lib import header_path
    assert int(re.search(r"#define VC_MHST_PCONV_CHUNK (\d+)", open(header_path()).read()).group(1)) == CHUNK


@pytest.mark.parametrize("name", list(CASES))
def test_pconv_family(name):
    B, D, C, O, G, KS, ldx, ycol, ldy = CASES[name]
    shape = (D, C, O, G, KS)
    assert L().vc_mhst_pconv_ok(*shape, ldx, ldy) == 1
    g = torch.Generator().manual_seed(1)
    x = rnd(g, B, C, D, 8, 8).requires_grad_(True)
    w = rnd(g, O, C // G, D, KS, KS).requires_grad_(True)
    bias = rnd(g, O).requires_grad_(True)
    dy = rnd(g, B, O, 1, 8, 8)
    y = F.conv3d(x, w, bias, padding=(0, KS // 2, KS // 2), groups=G)
    y.backward(dy)
    rows = lambda t: t.detach().permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])   # noqa: E731  channels-last rows
    Mo = B * 64
    xd = Poisoned(rows(x).float(), ld=ldx)
    wd = Poisoned(w.detach().reshape(1, -1).float(), lead=1)
    bd = Poisoned(bias.detach().reshape(1, -1).float(), lead=3)
    # dy's O columns at column ycol of rows of ldy, NaN in every other column
    dyw = torch.full((Mo, ldy), float("nan"))
    dyw[:, ycol:ycol + O] = rows(dy).float()
    dyd = Poisoned(dyw)
    dyp = dyd.ptr + 4 * ycol
    n = L().vc_mhst_pconv_ws_floats(B, *shape)
    ws = Guarded(1, n)

    def fwd(b):
        # the part's O columns start at column ycol of rows of ldy: everything else in the buffer must stay untouched
        flat = torch.full((Mo * ldy + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        L().vc_mhst_pconv_fwd(B, *shape, xd.ptr, ldx, wd.ptr, b, flat.data_ptr() + 4 * ycol, ldy, ws.ptr, n, stream())
        ws.check()
        flat = flat.cpu()
        got = flat.as_strided((Mo, O), (ldy, 1), ycol).clone()
        flat.as_strided((Mo, O), (ldy, 1), ycol).fill_(SENTINEL)
        assert bool((flat == SENTINEL).all()), "store outside the part's columns"
        return got

    got = fwd(bd.ptr)
    close("vc_mhst_pconv_fwd", name, got, rows(y))
    assert torch.equal(fwd(bd.ptr), got)      # a second run: the same bits
    close("vc_mhst_pconv_fwd no bias", name, fwd(None), rows(y) - bias.detach())

    init = rnd(g, B * D * 64, C).float()
    for beta in (0.0, 1.0):
        dxg = Guarded(B * D * 64, C, ld=ldx, init=init if beta else None)
        L().vc_mhst_pconv_dgrad(B, *shape, dyp, ldy, wd.ptr, dxg.ptr, ldx, beta, ws.ptr, n, stream())
        close("vc_mhst_pconv_dgrad", f"{name} beta {beta}", dxg.check(), rows(x.grad) + beta * init.double())
        ws.check()

    dwg, dbg = Guarded(1, w.numel()), Guarded(1, O)
    L().vc_mhst_pconv_wgrad(B, *shape, xd.ptr, ldx, dyp, ldy, dwg.ptr, dbg.ptr, ws.ptr, n, stream())
    got = dwg.check()
    ws.check()
    close("vc_mhst_pconv_wgrad", name, got, w.grad)
    close("vc_mhst_pconv_wgrad bias", name, dbg.check(), bias.grad)
    dwg = Guarded(1, w.numel())
    L().vc_mhst_pconv_wgrad(B, *shape, xd.ptr, ldx, dyp, ldy, dwg.ptr, None, ws.ptr, n, stream())
    assert torch.equal(dwg.check(), got)      # a second run, without db: the same bits
    ws.check()
