"""Every GLT-Net kernel (csrc/glt.hip) against float64 written from the formulas in include/vitcnn.h (tests/glt_oracle.py),
with guarded outputs and poisoned inputs, at the smallest shapes at which each can still go wrong.  Bound: 1e-4 of the
tensor's largest magnitude, the kernel classes' bound (DESIGN.md sections 16 and 22)."""
import pytest
import torch

import glt_oracle as O
from helpers import Guarded, Poisoned, within

pytestmark = pytest.mark.gpu
BOUND = 1e-4


def L():
    from vitcnn_amd._lib import lib
    return lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def rnd(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1


def close(kernel, shape, got, want):
    want = want.detach().reshape(got.shape)
    within(kernel, shape, float((got.double() - want).abs().max()), BOUND * max(float(want.abs().max()), 1e-30))


def rows(t):
    """[B, C, H, W] -> channels-last rows [B H W, C]"""
    return t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def scratch(n=1 << 20):
    return torch.empty(n, dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("B,C,P", [(1, 1, 2), (3, 5, 4), (2, 30, 8), (3, 11, 2), (1, 2, 8), (5, 3, 4)])
def test_crops(B, C, P):
    g = torch.Generator().manual_seed(B * 100 + C)
    x = rnd(g, B, C, 3 * P, 3 * P)
    ld = (C + 3) // 4 * 4
    xd = Poisoned(x.reshape(1, -1).float(), lead=1)
    out = [Guarded(B * (k * P) ** 2, ld) for k in (1, 2, 3)]
    L().vc_glt_crops(B, C, P, xd.ptr, out[0].ptr, out[1].ptr, out[2].ptr, ld, stream())
    for k, (o, want) in enumerate(zip(out, O.crops(x, P))):
        got = o.check()
        assert torch.equal(got[:, :C], rows(want).float()), k      # a copy: exact
        assert bool((got[:, C:] == 0).all()), k                    # the padding columns are zero-filled


def _fuse_case(B, P):
    """inputs whose SA-GDR maxima are pinned in float64 (runner-up >= 1e-5 below), the seed advancing until they are"""
    NP = P * P
    seed = 10 * P + B
    while True:
        g = torch.Generator().manual_seed(seed)
        pa = [rnd(g, B, 64, k * P // 2, k * P // 2).abs() for k in (1, 2, 3)]     # pooled ReLU outputs are >= 0
        pb = [rnd(g, B, 64, k * P // 2, k * P // 2).abs() for k in (1, 2, 3)]
        xs = rnd(g, 2) + 1.5
        W = [rnd(g, NP, (k * P // 2) ** 2) * 0.5 for k in (1, 2, 3)]
        bias = [rnd(g, NP) for _ in range(3)]
        w7, pos, cls = rnd(g, 1, 2, 7, 7) * 0.3, rnd(g, NP + 1, 64), rnd(g, 64)
        dX0, dxcnn = rnd(g, B, NP + 1, 64), rnd(g, B, NP, 64)
        leaves = pa + pb + [xs] + W + bias + [w7, pos, cls]
        for t in leaves:
            t.requires_grad_(True)
        xcnn, X0, e = O.fuse(pa, pb, xs[0], xs[1], W, bias, w7, pos, cls)
        top = e.detach().topk(2, dim=0).values
        if float((top[0] - top[1]).min()) >= 1e-5:
            break
        seed += 1000
    ((X0 * dX0).sum() + (xcnn * dxcnn).sum()).backward()
    return pa, pb, xs, W, bias, w7, pos, cls, dX0, dxcnn, xcnn, X0, e


@pytest.mark.parametrize("P", [2, 4, 8])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_fuse(B, P):
    NP, T = P * P, P * P + 1
    pa, pb, xs, W, bias, w7, pos, cls, dX0, dxcnn, xcnn, X0, e = _fuse_case(B, P)
    dev = lambda t, **kw: Poisoned(t.detach().float(), **kw)     # noqa: E731
    pad, pbd = [dev(rows(t)) for t in pa], [dev(rows(t)) for t in pb]
    xsd = dev(xs.reshape(1, 2), lead=1)
    Wd = [dev(t.reshape(1, -1), lead=k + 1) for k, t in enumerate(W)]
    bd = [dev(t.reshape(1, -1), lead=1) for t in bias]
    w7d, posd, clsd = dev(w7.reshape(1, -1), lead=3), dev(pos), dev(cls.reshape(1, -1), lead=2)
    xg, Xg, eg = Guarded(B * NP, 64), Guarded(B * T, 64), Guarded(3 * B * NP, 64)
    L().vc_glt_fuse_fwd(B, P, pad[0].ptr, pbd[0].ptr, pad[1].ptr, pbd[1].ptr, pad[2].ptr, pbd[2].ptr, xsd.ptr,
                        xsd.ptr + 4, Wd[0].ptr, bd[0].ptr, Wd[1].ptr, bd[1].ptr, Wd[2].ptr, bd[2].ptr, w7d.ptr, posd.ptr,
                        clsd.ptr, xg.ptr, Xg.ptr, eg.ptr, stream())
    shape = f"B={B} P={P}"
    close("vc_glt_fuse_fwd xcnn", shape, xg.check(), xcnn)
    close("vc_glt_fuse_fwd X0", shape, Xg.check(), X0)
    close("vc_glt_fuse_fwd e", shape, eg.check(), e.transpose(2, 3))
    # backward from the oracle's own saved tensors (what the forward wrote, to fp32)
    xcd, ed = dev(xcnn.reshape(B * NP, 64)), dev(e.transpose(2, 3).reshape(3 * B * NP, 64))
    dXd, dxd = dev(dX0.reshape(B * T, 64)), dev(dxcnn.reshape(B * NP, 64))
    width = L().vc_glt_fuse_part_floats(P)
    assert width == NP * (NP // 4 + NP + 9 * NP // 4) + 3 * NP + 100
    dpa = [Guarded(t.shape[0] * t.shape[2] * t.shape[3], 64) for t in pa]
    dpb = [Guarded(t.shape[0] * t.shape[2] * t.shape[3], 64) for t in pb]
    part = Guarded(B, width)
    L().vc_glt_fuse_bwd(B, P, pad[0].ptr, pbd[0].ptr, pad[1].ptr, pbd[1].ptr, pad[2].ptr, pbd[2].ptr, xsd.ptr, xsd.ptr + 4,
                        Wd[0].ptr, Wd[1].ptr, Wd[2].ptr, w7d.ptr, xcd.ptr, ed.ptr, dXd.ptr, dxd.ptr, dpa[0].ptr,
                        dpb[0].ptr, dpa[1].ptr, dpb[1].ptr, dpa[2].ptr, dpb[2].ptr, part.ptr, stream())
    for k in range(3):
        close(f"vc_glt_fuse_bwd dpa{k + 1}", shape, dpa[k].check(), rows(pa[k].grad))
        close(f"vc_glt_fuse_bwd dpb{k + 1}", shape, dpb[k].check(), rows(pb[k].grad))
    tot = part.check().double().sum(0)
    off = 0
    for k in range(3):
        n = W[k].numel()
        close(f"vc_glt_fuse_bwd dW{k + 1}", shape, tot[off:off + n], W[k].grad)
        close(f"vc_glt_fuse_bwd db{k + 1}", shape, tot[off + n:off + n + NP], bias[k].grad)
        off += n + NP
    close("vc_glt_fuse_bwd dw7", shape, tot[off:off + 98], w7.grad)
    close("vc_glt_fuse_bwd dxs", shape, tot[off + 98:off + 100], xs.grad)


@pytest.mark.parametrize("P", [2, 4, 8])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_tail(B, P):
    HW = P * P
    for n in (1, 12, 16, 70):
        g = torch.Generator().manual_seed(n + B)
        lg1, z = rnd(g, B, n).requires_grad_(True), rnd(g, B, HW, 32).requires_grad_(True)
        W2, b2, c = rnd(g, n, 32).requires_grad_(True), rnd(g, n).requires_grad_(True), rnd(g, 2).requires_grad_(True)
        dout = rnd(g, B, n)
        out = O.tail(lg1, z, W2, b2, c[0], c[1])
        out.backward(dout)
        dev = lambda t, **kw: Poisoned(t.detach().float(), **kw)     # noqa: E731
        lgd, zd = dev(lg1, lead=1), dev(z.reshape(B * HW, 32), ld=36)
        Wd, bd, cd = dev(W2.reshape(1, -1), lead=2), dev(b2.reshape(1, -1), lead=1), dev(c.reshape(1, 2), lead=3)
        p2, avg, og = Guarded(B, n), Guarded(B, 32), Guarded(B, n)
        L().vc_glt_tail_fwd(B, n, HW, lgd.ptr, zd.ptr, 36, Wd.ptr, bd.ptr, cd.ptr, cd.ptr + 4, p2.ptr, avg.ptr, og.ptr,
                            stream())
        shape = f"B={B} HW={HW} ncls={n}"
        close("vc_glt_tail_fwd", shape, og.check(), out)
        p2c, avgc = p2.check(), avg.check()
        close("vc_glt_tail_fwd avg", shape, avgc, z.mean(1))
        dlg, dz, part = Guarded(B, n), Guarded(B * HW, 32, ld=35), Guarded(B, n * 33 + 2)
        dod, p2d, avd = dev(dout), dev(p2c), dev(avgc)
        L().vc_glt_tail_bwd(B, n, HW, dod.ptr, lgd.ptr, p2d.ptr, avd.ptr, Wd.ptr, cd.ptr, cd.ptr + 4, dlg.ptr, dz.ptr, 35,
                            part.ptr, stream())
        close("vc_glt_tail_bwd dlg1", shape, dlg.check(), lg1.grad)
        close("vc_glt_tail_bwd dz", shape, dz.check(), z.grad.reshape(B * HW, 32))
        tot = part.check().double().sum(0)
        close("vc_glt_tail_bwd dW2", shape, tot[:n * 32], W2.grad)
        close("vc_glt_tail_bwd db2", shape, tot[n * 32:n * 33], b2.grad)
        close("vc_glt_tail_bwd dc", shape, tot[n * 33:], c.grad)


# every O (ragged against the 128-wide MFMA tile and the 4-float padding; 4, 72 and 144 take the pipelined kernel, whose
# tiles are 64 wide) and both batch sizes appear at every (P, s)
UP_CASES = [(1, 1), (2, 3), (3, 1), (5, 3), (11, 1), (30, 3), (4, 1), (72, 3), (144, 1)]


@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("P", [2, 4, 8])
def test_upconv(P, s):
    """forward, weight / bias gradient and data gradient (beta 0 and 1) against float64; the forward also against the
    existing vc_conv3x3_tap_fwd_ex on the materialised (repeat_interleave) input.  At P = 2, s = 3 every output pixel is
    within one tap of the zero border and of a replica edge."""
    C, SP = 64, s * P
    ws = scratch()
    for O_, B in UP_CASES:
        g = torch.Generator().manual_seed(1000 * P + 100 * s + O_)
        x = rnd(g, B, C, P, P).requires_grad_(True)
        w = (rnd(g, O_, C, 3, 3) * 0.2).requires_grad_(True)
        bias = rnd(g, O_).requires_grad_(True)
        dy = rnd(g, B, O_, SP, SP)
        y = O.upconv(x, w, bias, s)
        y.backward(dy)
        shape = f"P={P} s={s} O={O_} B={B}"
        ldy = (O_ + 3) // 4 * 4
        xd = Poisoned(rows(x).float(), ld=68)
        wt = torch.empty(O_ * 9 * C, dtype=torch.float32, device="cuda")
        wsrc = Poisoned(w.detach().reshape(1, -1).float(), lead=1)
        L().vc_conv3x3_pack(O_, C, 0, wsrc.ptr, wt.data_ptr(), 0.0, stream())
        bd = Poisoned(bias.detach().reshape(1, -1).float(), lead=3)
        for wsp, wsn in ((ws.data_ptr(), ws.numel()), (None, 0)):     # split-K slabs, and one pass
            yg = Guarded(B * SP * SP, O_, ld=ldy)
            L().vc_glt_upconv_fwd(B, P, s, C, O_, xd.ptr, 68, wt.data_ptr(), bd.ptr, yg.ptr, ldy, wsp, wsn, stream())
            got = yg.check()
            close("vc_glt_upconv_fwd", shape, got, rows(y))
        # the same convolution composed from the existing entry point on the materialised upsampled tensor
        up = x.detach().repeat_interleave(s, 2).repeat_interleave(s, 3)
        ud = Poisoned(rows(up).float(), ld=64)
        y2 = Guarded(B * SP * SP, O_, ld=ldy)
        L().vc_conv3x3_tap_fwd_ex(B, SP, SP, C, O_, 1, ud.ptr, 64, wt.data_ptr(), bd.ptr, y2.ptr, ldy, ws.data_ptr(),
                                  ws.numel(), 0, stream())
        ref = y2.check()
        within("vc_glt_upconv_fwd vs materialised", shape, float((got - ref).abs().max()),
               BOUND * float(ref.abs().max()))
        dyd = Poisoned(rows(dy).float(), ld=ldy + 4)
        for wsp, wsn in ((ws.data_ptr(), ws.numel()), (None, 0)):
            dwg, dbg = Guarded(1, w.numel()), Guarded(1, O_)
            L().vc_glt_upconv_wgrad(B, P, s, C, O_, xd.ptr, 68, dyd.ptr, ldy + 4, dwg.ptr, dbg.ptr, wsp, wsn, stream())
            close("vc_glt_upconv_wgrad", shape, dwg.check(), w.grad)
            close("vc_glt_upconv_wgrad bias", shape, dbg.check(), bias.grad)
        init = rnd(g, B * P * P, C).float()
        for beta in (0.0, 1.0):
            dxg = Guarded(B * P * P, C, ld=68, init=init if beta else None)
            L().vc_glt_upconv_dgrad(B, P, s, C, O_, dyd.ptr, ldy + 4, wt.data_ptr(), beta, dxg.ptr, 68, ws.data_ptr(),
                                    ws.numel(), stream())
            close("vc_glt_upconv_dgrad", f"{shape} beta {beta}", dxg.check(), rows(x.grad) + beta * init.double())


# element counts around the block's 2048 and its multiples; rows of C floats in a wider leading dimension
@pytest.mark.parametrize("R,C", [(1, 1), (7, 3), (2047, 1), (2048, 1), (2049, 1), (683, 3), (1024, 4), (1025, 4), (410, 5),
                                 (3 * 2048 + 1, 1), (576, 30)])
def test_sigmse(R, C):
    g = torch.Generator().manual_seed(R + C)
    y, t = (rnd(g, R, C) * 3).requires_grad_(True), rnd(g, R, C).abs()
    ld = (C + 3) // 4 * 4 + 4
    loss = O.sigmse(y, t) / 6
    loss.backward()
    nws = L().vc_glt_sigmse_ws_floats(R, C)
    assert nws == 2 * ((R * C + 2047) // 2048)
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    ws = scratch(nws + 2)
    td = Poisoned(t.float(), ld=ld)
    for acc, start in ((0, float("nan")), (1, 0.625)):
        yg = Guarded(R, C, ld=ld, init=y.detach().float())
        lg = Guarded(1, 1, init=torch.tensor([[start]]))
        L().vc_glt_sigmse_fwd(R, C, yg.ptr, ld, td.ptr, ld, 1.0 / 6.0, acc, lg.ptr, ws.data_ptr(), nws, cnt.data_ptr(),
                              stream())
        sg = yg.check()
        close("vc_glt_sigmse_fwd sigmoid", f"{R}x{C}", sg, torch.sigmoid(y))
        want = loss.detach() + (start if acc else 0.0)
        within("vc_glt_sigmse_fwd loss", f"{R}x{C} accumulate {acc}", abs(float(lg.check()) - float(want)),
               BOUND * float(want))
        assert not bool(cnt.any())      # the arrival counter is left zero
    dl = torch.tensor([0.75], device="cuda")
    sgd = Poisoned(sg, ld=ld)
    dg = Guarded(R, C, ld=ld)
    L().vc_glt_sigmse_bwd(R, C, sgd.ptr, ld, td.ptr, ld, 1.0 / 6.0, dl.data_ptr(), dg.ptr, ld, stream())
    close("vc_glt_sigmse_bwd", f"{R}x{C}", dg.check(), 0.75 * y.grad)
