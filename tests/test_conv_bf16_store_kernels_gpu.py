"""The tap-major 3x3 convs over bf16 operands stored in memory (vc_conv3x3_tap_fwd_h / _wgrad_oihw_h / _dgrad_h,
DESIGN.md section 30) against the yardstick of tests/test_fusat_bf16_kernels_gpu.py: the float64 conv and autograd over
bf16-ROUNDED x, w and dy, with the bias and the accumulated dx0 unrounded.  With the rounding factored out only the
fp32 accumulation is left, so the bounds are that file's own: max-relative 2e-6 sqrt(9 max(C, O)), norm-relative 3e-6,
db (vc_colsum_ex of the fp32 dy, as the model computes it in this mode) within 2e-6 sqrt(B OH OH) of the float64 column
sum of the unrounded dy.

The bf16 operands are made by the library's own producers (vc_cast_bf16_2d, vc_conv3x3_pack_bf16_many) inside buffers
whose every other element is a bf16 NaN -- beyond the last row of x16 / dy16 and behind the weight arena -- so a gather
that leaves an operand reaches a stored output as NaN; the pad columns [C, ld16) are the cast's zeros.  Shapes: ragged
C and O (ld16 40 / 56), one useful k per 64-wide tile, the 2193-channel concat (ld16 2200), one output tile with a
long K and a deep split-K, a valid conv and a 1x1 output; each with no workspace and with 4M floats of it."""
import pytest
import torch
import torch.nn.functional as F

from helpers import Guarded, Poisoned

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN16 = 0x7FC0   # a bf16 quiet NaN

SHAPES = [
    (2, 11, 37, 50, 1),      # ragged C and O, ld16 40 / 56
    (4, 11, 1, 16, 1),       # one useful k per tile (the 1-band LiDAR conv)
    (2, 11, 2193, 132, 1),   # the concat, ld16 = 2200
    (2, 5, 512, 64, 1),      # one output tile, long K, deep split-K
    (3, 7, 144, 256, 0),     # valid conv
    (4, 3, 256, 128, 0),     # 1x1 output
]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _nrel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def _r(t):
    return t.bfloat16().float()


def _up8(n):
    return (n + 7) // 8 * 8


def _reference(x, w, bias, dy, dx0, pad):
    """float64 conv + autograd over bf16-rounded x, w and (for the gradients) dy; bias, dx0 unrounded"""
    x64 = _r(x).double().permute(0, 3, 1, 2).requires_grad_(True)
    w64 = _r(w).double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, bias.double(), padding=pad)
    y64.backward(_r(dy).double().permute(0, 3, 1, 2))
    return (y64.detach().permute(0, 2, 3, 1), w64.grad, x64.grad.permute(0, 2, 3, 1) + dx0.double(),
            dy.double().sum(dim=(0, 1, 2)))


def _nan16(n):
    return torch.full((n,), NAN16, dtype=torch.int16, device=DEV)


class _Case:
    """one shape's fp32 inputs (Poisoned), their bf16 copies inside NaN-filled buffers, and the results of a run"""

    def __init__(self, B, H, C, O, pad, ws_log2, representable=False):
        from vitcnn_amd._lib import lib
        self.L = L = lib()
        self.geo = (B, H, C, O, pad)
        g = torch.Generator().manual_seed(B * 1000 + C + O)
        x = torch.randn(B, H, H, C, generator=g)
        w = torch.randn(O, C, 3, 3, generator=g) / (3 * C) ** 0.5
        bias = torch.randn(O, generator=g)
        OH = H + 2 * pad - 2
        dy = torch.randn(B, OH, OH, O, generator=g)
        dx0 = torch.randn(B, H, H, C, generator=g)
        if representable:   # operands that are bf16 values already: storing them as bf16 changes nothing
            x, w, dy = _r(x), _r(w), _r(dy)
        self.host = (x, w, bias, dy, dx0)
        self.OH = OH
        self.M, self.Mo = B * H * H, B * OH * OH
        self.xd = Poisoned(x.reshape(-1, C))
        self.dyd = Poisoned(dy.reshape(-1, O))
        self.bd = Poisoned(bias.reshape(1, O))
        self.wd = w.to(DEV).contiguous()
        self.s = s = torch.cuda.current_stream().cuda_stream
        self.ws = torch.empty(1 << ws_log2, device=DEV) if ws_log2 else None
        self.wsp, self.wsn = (self.ws.data_ptr(), self.ws.numel()) if ws_log2 else (None, 0)
        self.cws = torch.empty(1 << 16, device=DEV)   # the column sum's own partials
        # bf16 operands by the library's producers; NaN beyond the last row and behind the arena
        self.ldx, self.ldy = _up8(C), _up8(O)
        self.x16 = _nan16(self.M * self.ldx + 64)
        self.dy16 = _nan16(self.Mo * self.ldy + 64)
        self.wt16 = _nan16(O * 9 * self.ldx + 64)
        L.vc_cast_bf16_2d(self.M, C, self.xd.ptr, C, self.x16.data_ptr(), self.ldx, s)
        L.vc_cast_bf16_2d(self.Mo, O, self.dyd.ptr, O, self.dy16.data_ptr(), self.ldy, s)
        import ctypes
        shapes = (ctypes.c_int * 2)(O, C)
        src = (ctypes.c_void_p * 1)(self.wd.data_ptr())
        dst = (ctypes.c_void_p * 1)(self.wt16.data_ptr())
        L.vc_conv3x3_pack_bf16_many(1, ctypes.addressof(shapes), ctypes.addressof(src), ctypes.addressof(dst), s)
        torch.cuda.synchronize()
        for buf, n in ((self.x16, self.M * self.ldx), (self.dy16, self.Mo * self.ldy), (self.wt16, O * 9 * self.ldx)):
            assert bool((buf[n:] == NAN16).all()), "a producer wrote past its operand"

    def run(self):
        """(y, dw, db, dx) of the bf16-operand entry points"""
        B, H, C, O, pad = self.geo
        L, s = self.L, self.s
        dx0 = self.host[4]
        y = Guarded(self.Mo, O)
        dw = Guarded(O, 9 * C)
        db = Guarded(1, O)
        dx = Guarded(self.M, C, init=dx0.reshape(-1, C))
        x16, dy16, wt16 = self.x16.data_ptr(), self.dy16.data_ptr(), self.wt16.data_ptr()
        L.vc_conv3x3_tap_fwd_h(B, H, H, C, O, pad, x16, self.ldx, wt16, self.bd.ptr, y.ptr, O, self.wsp, self.wsn, s)
        L.vc_conv3x3_tap_wgrad_oihw_h(B, H, H, C, O, pad, x16, self.ldx, dy16, self.ldy, dw.ptr, self.wsp, self.wsn, s)
        L.vc_colsum_ex(self.Mo, O, self.dyd.ptr, O, db.ptr, 0.0, self.cws.data_ptr(), self.cws.numel(), None, 0, s)
        L.vc_conv3x3_tap_dgrad_h(B, H, H, C, O, pad, dy16, self.ldy, wt16, 1.0, dx.ptr, C, self.wsp, self.wsn, s)
        return (y.check().reshape(B, self.OH, self.OH, O), dw.check().reshape(O, C, 3, 3), db.check().reshape(O),
                dx.check().reshape(B, H, H, C))

    def run_fp32(self):
        """the plain fp32 entry points on the fp32 operands"""
        B, H, C, O, pad = self.geo
        L, s = self.L, self.s
        dx0 = self.host[4]
        Cw = (C + 3) // 4 * 4
        wt = torch.full((O * 9 * Cw + 64,), float("nan"), device=DEV)
        L.vc_conv3x3_pack(O, C, 0, self.wd.data_ptr(), wt.data_ptr(), 0.0, s)
        y = Guarded(self.Mo, O)
        dw = Guarded(O, 9 * C)
        db = Guarded(1, O)
        dx = Guarded(self.M, C, init=dx0.reshape(-1, C))
        L.vc_conv3x3_tap_fwd(B, H, H, C, O, pad, self.xd.ptr, C, wt.data_ptr(), self.bd.ptr, y.ptr, O, self.wsp,
                             self.wsn, s)
        L.vc_conv3x3_tap_wgrad_oihw(B, H, H, C, O, pad, self.xd.ptr, C, self.dyd.ptr, O, dw.ptr, db.ptr, self.wsp,
                                    self.wsn, s)
        L.vc_conv3x3_tap_dgrad(B, H, H, C, O, pad, self.dyd.ptr, O, wt.data_ptr(), 1.0, dx.ptr, C, self.wsp, self.wsn,
                               s)
        return (y.check().reshape(B, self.OH, self.OH, O), dw.check().reshape(O, C, 3, 3), db.check().reshape(O),
                dx.check().reshape(B, H, H, C))

    def bounds(self):
        B, H, C, O, pad = self.geo
        return 2e-6 * (9 * max(C, O)) ** 0.5, 3e-6, 2e-6 * (B * self.OH * self.OH) ** 0.5


def _errs(got, ref):
    y, dw, _, dx = got
    return ((_rel(y, ref[0]), _rel(dw, ref[1]), _rel(dx, ref[2])),
            (_nrel(y, ref[0]), _nrel(dw, ref[1]), _nrel(dx, ref[2])))


@pytest.mark.parametrize("B,H,C,O,pad", SHAPES)
@pytest.mark.parametrize("ws_log2", [0, 22])
def test_stored_bf16_conv_matches_float64_conv_of_rounded_operands(B, H, C, O, pad, ws_log2):
    _need_gpu()
    c = _Case(B, H, C, O, pad, ws_log2)
    x, w, bias, dy, dx0 = c.host
    ref = _reference(x, w, bias, dy, dx0, pad)
    got = c.run()
    tol, ntol, dbtol = c.bounds()
    mx, nr = _errs(got, ref)
    print("errs", mx, nr, "bounds", tol, ntol)
    assert max(mx) < tol, (mx, tol)
    assert max(nr) < ntol, nr
    # the bias gradient: the fp32 column sum of the UNROUNDED dy
    assert _rel(got[2], ref[3]) < dbtol, _rel(got[2], ref[3])
    # run-to-run bit-identical (split-K with ws_log2 = 22)
    again = c.run()
    for a, b in zip(again, got):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,H,C,O,pad", SHAPES)
@pytest.mark.parametrize("ws_log2", [0, 22])
def test_stored_bf16_conv_of_representable_operands_agrees_with_fp32(B, H, C, O, pad, ws_log2):
    """x, w, dy already bf16 values: storing them as bf16 changes nothing, so the result must agree with the fp32
    entry points (and the float64 conv) within the fp32 bounds -- a kernel that also rounds the bias, dx0 or an
    accumulator does not"""
    _need_gpu()
    c = _Case(B, H, C, O, pad, ws_log2, representable=True)
    x, w, bias, dy, dx0 = c.host
    ref = _reference(x, w, bias, dy, dx0, pad)
    got, fp = c.run(), c.run_fp32()
    tol, ntol, dbtol = c.bounds()
    for r in (got, fp):
        mx, nr = _errs(r, ref)
        print("errs", mx, nr, "bounds", tol, ntol)
        assert max(mx) < tol, (mx, tol)
        assert max(nr) < ntol, nr
        assert _rel(r[2], ref[3]) < dbtol
    for i in (0, 1, 3):   # and against each other, within the same bounds
        assert _rel(got[i], fp[i]) < tol, (i, _rel(got[i], fp[i]))
        assert _nrel(got[i], fp[i]) < ntol, (i, _nrel(got[i], fp[i]))


def test_argument_refusals_are_status_1():
    """ld16 % 8 != 0, a base that is not 16-B aligned and a null operand: status 1 (before any launch)"""
    _need_gpu()
    from vitcnn_amd._lib import lib
    L = lib()
    B, H, C, O, pad = 2, 5, 16, 16, 1
    s = torch.cuda.current_stream().cuda_stream
    a16 = torch.zeros(4096, dtype=torch.int16, device=DEV)   # >= O * 9 * 16 (Wt16) and B * H * H * 16 (x16, dy16)
    f32 = torch.zeros(B * H * H * 24 * 9, device=DEV)
    p16, pf = a16.data_ptr(), f32.data_ptr()

    def calls(x16, ldx, dy16, ldy, wt16):
        return (L.raw["vc_conv3x3_tap_fwd_h"](B, H, H, C, O, pad, x16, ldx, wt16, None, pf, O, None, 0, s),
                L.raw["vc_conv3x3_tap_wgrad_oihw_h"](B, H, H, C, O, pad, x16, ldx, dy16, ldy, pf, None, 0, s),
                L.raw["vc_conv3x3_tap_dgrad_h"](B, H, H, C, O, pad, dy16, ldy, wt16, 0.0, pf, C, None, 0, s))

    assert calls(p16, 16, p16, 16, p16) == (0, 0, 0)
    assert calls(p16, 20, p16, 20, p16) == (1, 1, 1)            # ld16 % 8 != 0
    assert calls(p16 + 2, 16, p16 + 2, 16, p16) == (1, 1, 1)    # misaligned x16 / dy16
    assert calls(p16, 16, p16, 16, p16 + 8)[::2] == (1, 1)      # misaligned Wt16
    assert calls(None, 16, None, 16, p16) == (1, 1, 1)          # null x16 / dy16
    assert calls(p16, 16, p16, 16, None)[::2] == (1, 1)         # null Wt16
    assert calls(p16, 8, p16, 8, p16) == (1, 1, 1)              # ld16 < C / O
    assert L.raw["vc_cast_bf16_2d"](4, 5, pf, 5, p16, 7, s) == 1
    assert L.raw["vc_cast_bf16_2d"](4, 5, pf, 5, p16 + 2, 8, s) == 1
    torch.cuda.synchronize()
