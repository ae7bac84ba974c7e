"""The tap-major 3x3 convs with VC_CONV_BF16 (vc_conv3x3_tap_fwd_ex / _wgrad_ex / _wgrad_oihw_ex / _dgrad_ex, flags 2)
against the float64 conv of tests/test_conv_tap_gpu.py applied to bf16-ROUNDED operands: the forward of rounded x and
w, the weight gradient of rounded dy and x, the data gradient of rounded dy and w; bias, the accumulated dx0 and the
bias gradient are unrounded.  With the rounding factored out only the fp32 accumulation is left, so the bounds are
the fp32 kernels' own: max-relative 2e-6 sqrt(9 max(C, O)), norm-relative 3e-6, db within 2e-6 sqrt(B OH OH) of the
column sum of the unrounded dy.  The shapes are the smallest that reach both kernels, the concat with C % 4 != 0 on
each of them, a deep split-K, valid convs and a 1x1 output.  Which kernel takes a shape is conv_pipe_ok's rule
(conv_tap.hip): conv_pipe needs O and both leading dimensions (ldx; ldy = lddy = O here) to be multiples of 4 and
16-B aligned bases, in all three directions alike; everything else goes to conv_tap."""
import pytest
import torch
import torch.nn.functional as F

from helpers import Guarded, Poisoned

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = 2   # VC_CONV_BF16

SHAPES = [
    (2, 11, 37, 50, 1, 37),        # conv_tap (ldx = 37, O = 50): ragged channels, scalar loads
    (4, 11, 1, 16, 1, 1),          # conv_tap (ldx = 1): the 1-band LiDAR conv
    (2, 11, 2193, 130, 1, 2196),   # conv_tap (O = 130 is no multiple of 4): the concat, float4 loads masked at C
    (2, 11, 2193, 132, 1, 2196),   # conv_pipe (O = 132): the concat with C % 4 != 0 -- the last 16-B chunk of a row
                                   # reads the finite garbage in x[:, C:ldx], which must meet the zero weight padding
    (2, 5, 512, 64, 1, 512),       # conv_pipe: one output tile, long K, deep split-K
    (3, 7, 144, 256, 0, 144),      # conv_pipe: valid conv
    (4, 3, 256, 128, 0, 256),      # conv_pipe: 3x3 -> 1x1 output
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


def _reference(x, w, bias, dy, dx0, pad):
    """float64 conv + autograd over bf16-rounded x, w and (for the gradients) dy; bias, dx0 unrounded"""
    x64 = _r(x).double().permute(0, 3, 1, 2).requires_grad_(True)
    w64 = _r(w).double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, bias.double(), padding=pad)
    y64.backward(_r(dy).double().permute(0, 3, 1, 2))
    return (y64.detach().permute(0, 2, 3, 1), w64.grad, x64.grad.permute(0, 2, 3, 1) + dx0.double(),
            dy.double().sum(dim=(0, 1, 2)))


class _Case:
    """one shape's inputs on the device (Poisoned) and the four results of one flags value"""

    def __init__(self, B, H, C, O, pad, ldx, ws_log2, representable=False):
        from vitcnn_amd._lib import lib
        self.L = lib()
        self.geo = (B, H, C, O, pad, ldx)
        g = torch.Generator().manual_seed(B * 1000 + C + O)
        x = torch.randn(B, H, H, C, generator=g)
        w = torch.randn(O, C, 3, 3, generator=g) / (3 * C) ** 0.5
        bias = torch.randn(O, generator=g)
        OH = H + 2 * pad - 2
        dy = torch.randn(B, OH, OH, O, generator=g)
        dx0 = torch.randn(B, H, H, C, generator=g)
        if representable:   # operands that are bf16 values already: the flag may change nothing but the MFMA
            x, w, dy = _r(x), _r(w), _r(dy)
        self.host = (x, w, bias, dy, dx0)
        self.OH = OH
        # with C % 4 != 0 and ldx % 4 == 0 the pipelined kernel reads the row padding up to C rounded to 4 against zero
        # weights (include/vitcnn.h: finite values there, so finite garbage; conv_tap on the O = 130 shape never reads
        # it); everything else outside the operands is NaN
        finite = C % 4 and ldx % 4 == 0
        self.xd = Poisoned(x.reshape(-1, C), ld=ldx, poison=3.0 if finite else float("nan"))
        self.dyd = Poisoned(dy.reshape(-1, O))
        self.bd = Poisoned(bias.reshape(1, O))
        self.wd = w.to(DEV).contiguous()
        self.s = torch.cuda.current_stream().cuda_stream
        self.ws = torch.empty(1 << ws_log2, device=DEV) if ws_log2 else None
        self.wsp, self.wsn = (self.ws.data_ptr(), self.ws.numel()) if ws_log2 else (None, 0)
        Cw = (C + 3) // 4 * 4
        self.wt = torch.full((O * 9 * Cw + 64,), float("nan"), device=DEV)   # NaN past the packed weights
        self.L.vc_conv3x3_pack(O, C, 0, self.wd.data_ptr(), self.wt.data_ptr(), 0.0, self.s)

    def run(self, flags, plain=False):
        """(y, dw via wgrad + pack, dw via _oihw, db, dx); plain: the entry points without `flags`"""
        B, H, C, O, pad, ldx = self.geo
        L, s, OH = self.L, self.s, self.OH
        x, w, bias, dy, dx0 = self.host
        M = B * OH * OH
        y = Guarded(M, O)
        dwt = Guarded(O, 9 * C)
        dw2 = Guarded(O, 9 * C)
        db = Guarded(1, O)
        dx = Guarded(B * H * H, C, ld=ldx, init=dx0.reshape(-1, C))
        a_f = (B, H, H, C, O, pad, self.xd.ptr, ldx, self.wt.data_ptr(), self.bd.ptr, y.ptr, O, self.wsp, self.wsn)
        a_w = (B, H, H, C, O, pad, self.xd.ptr, ldx, self.dyd.ptr, O, dwt.ptr, self.wsp, self.wsn)
        a_o = (B, H, H, C, O, pad, self.xd.ptr, ldx, self.dyd.ptr, O, dw2.ptr, db.ptr, self.wsp, self.wsn)
        a_d = (B, H, H, C, O, pad, self.dyd.ptr, O, self.wt.data_ptr(), 1.0, dx.ptr, ldx, self.wsp, self.wsn)
        if plain:
            L.vc_conv3x3_tap_fwd(*a_f, s)
            L.vc_conv3x3_tap_wgrad(*a_w, s)
            L.vc_conv3x3_tap_wgrad_oihw(*a_o, s)
            L.vc_conv3x3_tap_dgrad(*a_d, s)
        else:
            L.vc_conv3x3_tap_fwd_ex(*a_f, flags, s)
            L.vc_conv3x3_tap_wgrad_ex(*a_w, flags, s)
            L.vc_conv3x3_tap_wgrad_oihw_ex(*a_o, flags, s)
            L.vc_conv3x3_tap_dgrad_ex(*a_d, flags, s)
        dwt_out = dwt.check()
        dw = torch.full((O, C, 3, 3), 7.0, device=DEV)
        L.vc_conv3x3_pack(O, C, 2, dwt.ptr, dw.data_ptr(), 0.0, s)
        # Guarded.check: gap columns (dx[:, C:]) and guards untouched
        return (y.check().reshape(B, OH, OH, O), dw.cpu(), dw2.check().reshape(O, C, 3, 3), db.check().reshape(O),
                dx.check().reshape(B, H, H, C), dwt_out)

    def bounds(self):
        B, H, C, O, pad, ldx = self.geo
        return 2e-6 * (9 * max(C, O)) ** 0.5, 3e-6, 2e-6 * (B * self.OH * self.OH) ** 0.5


def _errs(got, ref):
    y, dw, _, _, dx, _ = got
    return ((_rel(y, ref[0]), _rel(dw, ref[1]), _rel(dx, ref[2])),
            (_nrel(y, ref[0]), _nrel(dw, ref[1]), _nrel(dx, ref[2])))


@pytest.mark.parametrize("B,H,C,O,pad,ldx", SHAPES)
@pytest.mark.parametrize("ws_log2", [0, 22])
def test_bf16_conv_matches_float64_conv_of_rounded_operands(B, H, C, O, pad, ldx, ws_log2):
    _need_gpu()
    c = _Case(B, H, C, O, pad, ldx, ws_log2)
    x, w, bias, dy, dx0 = c.host
    ref = _reference(x, w, bias, dy, dx0, pad)
    got = c.run(BF16)
    tol, ntol, dbtol = c.bounds()
    mx, nr = _errs(got, ref)
    print("errs", mx, nr, "bounds", tol, ntol)
    assert max(mx) < tol, (mx, tol)
    assert max(nr) < ntol, nr
    # the bias gradient: the fp32 column sum of the UNROUNDED dy
    assert _rel(got[3], ref[3]) < dbtol, _rel(got[3], ref[3])
    # straight into the torch layout: bit-identical to wgrad + pack mode 2, as the fp32 pair
    assert torch.equal(got[2], got[1])
    # the flag is in effect: the fp32 entry points give another result on the same inputs
    fp = c.run(0, plain=True)
    for i in (0, 1, 4):
        assert not torch.equal(got[i], fp[i]), i
    assert torch.equal(got[3], fp[3])   # db: the same fp32 sum of the same dy
    # flags 0 is the plain entry point, bit for bit
    ex0 = c.run(0)
    for a, b in zip(ex0, fp):
        assert torch.equal(a, b)
    # a bf16 conv (split-K with ws_log2 = 22) is run-to-run bit-identical
    again = c.run(BF16)
    for a, b in zip(again, got):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,H,C,O,pad,ldx", SHAPES)
@pytest.mark.parametrize("ws_log2", [0, 22])
def test_bf16_conv_of_representable_operands_agrees_with_fp32(B, H, C, O, pad, ldx, ws_log2):
    """x, w, dy already bf16 values: rounding them changes nothing, so the bf16 result must agree with the fp32 entry
    points (and the float64 conv) within the fp32 bounds -- a kernel that also rounds the bias, dx0 or an accumulator
    does not"""
    _need_gpu()
    c = _Case(B, H, C, O, pad, ldx, ws_log2, representable=True)
    x, w, bias, dy, dx0 = c.host
    ref = _reference(x, w, bias, dy, dx0, pad)
    got, fp = c.run(BF16), c.run(0, plain=True)
    tol, ntol, dbtol = c.bounds()
    for r in (got, fp):
        mx, nr = _errs(r, ref)
        print("errs", mx, nr, "bounds", tol, ntol)
        assert max(mx) < tol, (mx, tol)
        assert max(nr) < ntol, nr
        assert _rel(r[3], ref[3]) < dbtol
    for i in (0, 1, 4):   # and against each other, within the same bounds
        assert _rel(got[i], fp[i]) < tol, (i, _rel(got[i], fp[i]))
        assert _nrel(got[i], fp[i]) < ntol, (i, _nrel(got[i], fp[i]))
    assert torch.equal(got[3], fp[3])
