"""Per-kernel parity of csrc/mft.hip on the MI355X: each entry point against float64 written here from the formulas
in include/vitcnn.h, at the smallest shapes at which it can go wrong (depth 1, odd and even patch widths, several
depth chunks, both HetConv group counts, one channel per group, 1 and 4 tokens, 2 / 5 / 16 attention rows).

Outputs start as NaN and are followed by a guard region (helpers.Guarded) that must stay untouched.
Tolerances: the 3-D conv takes test_conv_tap_gpu.py's classes (its tol 2e-6 sqrt(9 max(C, O)) at (C, O) = (1, 8),
1.7e-5, for the forward and the weight gradient; 2e-6 sqrt(count) for the bias gradient); pack / unpack are
bit-exact; token pooling and the attention core: 1e-4 of the reference's max |value| (the reduction / attention
class of test_s2eft_kernels_gpu.py); the broadcast residual: rel_err < 1e-6.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import Guarded, rel_err, within

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vitcnn_amd._lib import lib
    return lib()


def S():
    return torch.cuda.current_stream().cuda_stream


def uni(*shape, seed=0, lo=-1.0, hi=1.0, scale=0.97130763):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * (hi - lo) + lo) * scale


# ---------------------------------------------------------------------------------------------- conv5 (3-D conv)
@pytest.mark.parametrize("B,NC,P", [(2, 9, 5), (3, 11, 7), (2, 30, 11), (1, 13, 6)])
def test_conv3d_fwd_wgrad(L, B, NC, P):
    """vc_mft_conv3d_fwd / _wgrad against F.conv3d in float64; rows [B P P, ld] with channel d*8 + c, a padded
    leading dimension whose gap columns must stay untouched"""
    D = NC - 8
    C6 = 8 * D
    ld = C6 + 4
    x = uni(B, NC, P, P, seed=NC)
    w = uni(8, 1, 9, 3, 3, seed=NC + 1) / 9.0
    bias = uni(8, seed=NC + 2)
    dy = uni(B, 8, D, P, P, seed=NC + 3)
    x64, w64, b64 = x.double(), w.double().requires_grad_(True), bias.double().requires_grad_(True)
    y64 = F.conv3d(x64.unsqueeze(1), w64, b64, padding=(0, 1, 1))      # [B, 8, D, P, P]
    y64.backward(dy.double())
    to_rows = lambda t: t.permute(0, 3, 4, 2, 1).reshape(B * P * P, C6)   # [b, h, w, d, c]
    xd, wd, bd = x.to(DEV), w.to(DEV).contiguous(), bias.to(DEV)
    y = Guarded(B * P * P, C6, ld=ld)
    L.vc_mft_conv3d_fwd(B, NC, P, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.ptr, ld, S())
    tol = 2e-6 * (9 * max(1, 8)) ** 0.5   # test_conv_tap_gpu.py's tol at (C, O) = (1, 8)
    within("vc_mft_conv3d_fwd", (B, NC, P), rel_err(y.check(), to_rows(y64.detach())), tol)
    dyd = torch.full((B * P * P, ld), float("nan"), device=DEV)
    dyd[:, :C6] = to_rows(dy).to(DEV)
    n_ws = L.vc_mft_conv3d_ws_floats(B, NC, P)
    ws = torch.empty(n_ws, device=DEV)
    dw, db = Guarded(8, 81), Guarded(1, 8)
    L.vc_mft_conv3d_wgrad(B, NC, P, xd.data_ptr(), dyd.data_ptr(), ld, dw.ptr, db.ptr, ws.data_ptr(), n_ws, S())
    within("vc_mft_conv3d_wgrad dw", (B, NC, P), rel_err(dw.check(), w64.grad.reshape(8, 81)), tol)
    within("vc_mft_conv3d_wgrad db", (B, NC, P), rel_err(db.check()[0], b64.grad), 2e-6 * (B * D * P * P) ** 0.5)
    # a workspace one float short is refused before any launch
    assert L.raw["vc_mft_conv3d_wgrad"](B, NC, P, xd.data_ptr(), dyd.data_ptr(), ld, dw.ptr, db.ptr, ws.data_ptr(),
                                        n_ws - 1, S()) == 1


# ---------------------------------------------------------------------------------------------- conv6 (HetConv)
@pytest.mark.parametrize("g,cpg", [(16, 11), (8, 3), (8, 1)])
def test_hetconv_pack_unpack_bit_exact(L, g, cpg):
    """vc_mft_hetconv_pack / _unpack: copies and one add, so bit-exact; entries off the group diagonal are exactly
    zero after pack, and unpack ignores them"""
    O, C = 64, g * cpg
    D = C // 8
    gw, pw = uni(O, cpg, 3, 3, seed=g + cpg), uni(O, C, seed=g + cpg + 1)
    gb, pb = uni(O, seed=3), uni(O, seed=4)
    dense = torch.zeros(O, C, 3, 3)          # torch channel order
    opg = O // g
    for o in range(O):
        grp = o // opg
        dense[o, grp * cpg:(grp + 1) * cpg] = gw[o]
    on_diag = dense != 0
    dense[:, :, 1, 1] = dense[:, :, 1, 1] + pw
    ch = torch.arange(C)
    col = (ch % D) * 8 + ch // D             # torch channel ch = c D + d  ->  column d*8 + c
    ref = torch.zeros(O, 9, C)
    ref[:, :, col] = dense.reshape(O, C, 9).permute(0, 2, 1)
    wt, bias = Guarded(O * 9, C), Guarded(1, O)
    d = lambda t: t.to(DEV).contiguous()
    gwd, pwd, gbd, pbd = d(gw), d(pw), d(gb), d(pb)
    L.vc_mft_hetconv_pack(O, C, g, gwd.data_ptr(), pwd.data_ptr(), gbd.data_ptr(), pbd.data_ptr(), wt.ptr, bias.ptr, S())
    got = wt.check().reshape(O, 9, C)
    assert torch.equal(got, ref)
    assert torch.equal(bias.check()[0], gb + pb)
    off = torch.ones(O, 9, C, dtype=torch.bool)
    off[:, :, col] = on_diag.reshape(O, C, 9).permute(0, 2, 1)
    off[:, 4, :] = True                      # the centre tap holds pwc everywhere
    assert bool((got[~off] == 0).all()) and int((~off).sum()) == O * 8 * (C - cpg)
    # unpack: a dense gradient with values everywhere; the off-diagonal ones must not reach the outputs
    dwt = uni(O, 9, C, seed=9)
    dd = dwt[:, :, col].permute(0, 2, 1).reshape(O, C, 3, 3)     # back in the torch channel order
    dgw_ref = torch.stack([dd[o, (o // opg) * cpg:(o // opg + 1) * cpg] for o in range(O)])
    dpw_ref = dd[:, :, 1, 1]
    dgw, dpw = Guarded(O * cpg, 9), Guarded(O, C)
    dwtd = d(dwt)
    L.vc_mft_hetconv_unpack(O, C, g, dwtd.data_ptr(), dgw.ptr, dpw.ptr, S())
    assert torch.equal(dgw.check().reshape(O, cpg, 3, 3), dgw_ref)
    assert torch.equal(dpw.check(), dpw_ref)


# ---------------------------------------------------------------------------------------------- tokenisers
@pytest.mark.parametrize("Lt", [1, 4])
@pytest.mark.parametrize("HW", [25, 49, 121])
@pytest.mark.parametrize("B", [1, 3])
def test_tokpool_fwd_bwd(L, Lt, HW, B):
    """vc_mft_tokpool_fwd / _bwd: rows with a padded leading dimension, the tokens written into rows 1.. of a
    [B, 5, 64] token buffer (the model's layout) with the position rows added"""
    ldx, T = 68, 5
    X = uni(B, HW, 64, seed=HW + Lt)
    wA, wV, add = uni(Lt, 64, seed=1) * 0.5, uni(64, 64, seed=2) * 0.2, uni(Lt, 64, seed=3)
    dT = uni(B, Lt, 64, seed=4)
    X64 = X.double().requires_grad_(True)
    wA64, wV64 = wA.double().requires_grad_(True), wV.double().requires_grad_(True)
    A64 = torch.softmax(torch.einsum("lj,bij->bli", wA64, X64), dim=-1)
    U64 = A64 @ X64
    T64 = A64 @ (X64 @ wV64) + add.double()
    T64.backward(dT.double())
    Xd = torch.full((B * HW, ldx), float("nan"), device=DEV)
    Xd[:, :64] = X.reshape(-1, 64).to(DEV)
    wAd, wVd, addd = wA.to(DEV), wV.to(DEV), add.to(DEV)
    A, U = Guarded(B * Lt, HW), Guarded(B * Lt, 64)
    tok = Guarded(B * T, 64)
    row0 = T - Lt
    L.vc_mft_tokpool_fwd(B, HW, Lt, Xd.data_ptr(), ldx, wAd.data_ptr(), wVd.data_ptr(), addd.data_ptr(), A.ptr, U.ptr,
                         tok.ptr + 4 * 64 * row0, 64, T * 64, S())
    shape = (B, HW, Lt)
    within("vc_mft_tokpool_fwd A", shape, rel_err(A.check().reshape(B, Lt, HW), A64.detach()), 1e-4)
    within("vc_mft_tokpool_fwd U", shape, rel_err(U.check().reshape(B, Lt, 64), U64.detach()), 1e-4)
    got = tok.check().reshape(B, T, 64)
    within("vc_mft_tokpool_fwd T", shape, rel_err(got[:, row0:], T64.detach()), 1e-4)
    assert torch.isnan(got[:, :row0]).all()   # the other token rows are not this call's
    # backward from dT laid out in the same token rows
    dTd = torch.full((B, T, 64), float("nan"), device=DEV)
    dTd[:, row0:] = dT.to(DEV)
    dX = Guarded(B * HW, 64, ld=ldx)
    dwA, dwV = Guarded(Lt, 64), Guarded(64, 64)
    n_ws = B * (Lt * 64 + 4096)
    ws = torch.empty(n_ws, device=DEV)
    Ad, Ud = A.view.contiguous(), U.view.contiguous()
    L.vc_mft_tokpool_bwd(B, HW, Lt, Xd.data_ptr(), ldx, wAd.data_ptr(), wVd.data_ptr(), Ad.data_ptr(), Ud.data_ptr(),
                         dTd.data_ptr() + 4 * 64 * row0, 64, T * 64, dX.ptr, ldx, dwA.ptr, dwV.ptr, ws.data_ptr(),
                         n_ws, S())
    within("vc_mft_tokpool_bwd dX", shape, rel_err(dX.check().reshape(B, HW, 64), X64.grad), 1e-4)
    within("vc_mft_tokpool_bwd dwA", shape, rel_err(dwA.check(), wA64.grad), 1e-4)
    within("vc_mft_tokpool_bwd dwV", shape, rel_err(dwV.check(), wV64.grad), 1e-4)
    assert L.raw["vc_mft_tokpool_bwd"](B, HW, Lt, Xd.data_ptr(), ldx, wAd.data_ptr(), wVd.data_ptr(), Ad.data_ptr(),
                                       Ud.data_ptr(), dTd.data_ptr(), 64, T * 64, dX.ptr, ldx, dwA.ptr, dwV.ptr,
                                       ws.data_ptr(), n_ws - 1, S()) == 1


# ---------------------------------------------------------------------------------------------- cross attention
@pytest.mark.parametrize("T", [2, 5, 16])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_xattn_fwd_bwd(L, T, B):
    """vc_mft_xattn_fwd / _bwd against the formula in float64; the weight gradients are bit-identical across runs"""
    Y = uni(B, T, 64, seed=T + B) * 2.0
    wq, wk, wv = uni(64, 8, seed=1), uni(64, 8, seed=2), uni(64, 8, seed=3)
    dO = uni(B, 512, seed=4)
    scale = 8 ** -0.5
    Y64 = Y.double().requires_grad_(True)
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (wq, wk, wv))
    ys = Y64.reshape(B, T, 8, 8)
    q = (ys[:, 0:1] @ q64.t()).permute(0, 2, 1, 3)
    k = (ys @ k64.t()).permute(0, 2, 1, 3)
    v = (ys @ v64.t()).permute(0, 2, 1, 3)
    a64 = torch.softmax((q @ k.transpose(-2, -1)) * scale, dim=-1)     # [B, 8, 1, T]
    O64 = (a64 @ v).transpose(1, 2).reshape(B, 512)
    O64.backward(dO.double())
    Yd, wqd, wkd, wvd, dOd = (t.to(DEV).contiguous() for t in (Y, wq, wk, wv, dO))
    O, att = Guarded(B, 512), Guarded(B * 8, T)
    L.vc_mft_xattn_fwd(B, T, Yd.data_ptr(), wqd.data_ptr(), wkd.data_ptr(), wvd.data_ptr(), scale, O.ptr, att.ptr, S())
    within("vc_mft_xattn_fwd O", (B, T), rel_err(O.check(), O64.detach()), 1e-4)
    within("vc_mft_xattn_fwd attn", (B, T), rel_err(att.check().reshape(B, 8, 1, T), a64.detach()), 1e-4)
    n_ws = B * 1536
    ws = torch.empty(n_ws, device=DEV)
    attd = att.view.contiguous()
    runs = []
    for _ in range(2):
        dY, dq, dk, dv = Guarded(B * T, 64), Guarded(64, 8), Guarded(64, 8), Guarded(64, 8)
        L.vc_mft_xattn_bwd(B, T, Yd.data_ptr(), wqd.data_ptr(), wkd.data_ptr(), wvd.data_ptr(), attd.data_ptr(),
                           dOd.data_ptr(), scale, dY.ptr, dq.ptr, dk.ptr, dv.ptr, ws.data_ptr(), n_ws, S())
        runs.append((dY.check(), dq.check(), dk.check(), dv.check()))
    dY, dq, dk, dv = runs[0]
    within("vc_mft_xattn_bwd dY", (B, T), rel_err(dY.reshape(B, T, 64), Y64.grad), 1e-4)
    within("vc_mft_xattn_bwd dwq", (B, T), rel_err(dq, q64.grad), 1e-4)
    within("vc_mft_xattn_bwd dwk", (B, T), rel_err(dk, k64.grad), 1e-4)
    within("vc_mft_xattn_bwd dwv", (B, T), rel_err(dv, v64.grad), 1e-4)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- broadcast residual
@pytest.mark.parametrize("B,T,D", [(3, 5, 64), (1, 2, 7), (64, 5, 64)])
def test_bcast_add_fwd_bwd(L, B, T, D):
    h, a, dout = uni(B, T, D, seed=1), uni(B, D, seed=2), uni(B, T, D, seed=3)
    hd, ad, dd = h.to(DEV), a.to(DEV), dout.to(DEV)
    out, da = Guarded(B * T, D), Guarded(B, D)
    L.vc_mft_bcast_add_fwd(B, T, D, hd.data_ptr(), ad.data_ptr(), out.ptr, S())
    L.vc_mft_bcast_add_bwd(B, T, D, dd.data_ptr(), da.ptr, S())
    within("vc_mft_bcast_add_fwd", (B, T, D), rel_err(out.check().reshape(B, T, D), h.double() + a.double()[:, None]),
           1e-6)
    within("vc_mft_bcast_add_bwd", (B, T, D), rel_err(da.check(), dout.double().sum(1)), 1e-6)


# ---------------------------------------------------------------------------------------------- Adam, coupled L2
@pytest.mark.parametrize("n", [1003, 4096 + 5])
def test_adam_one_step_against_the_formula(L, n):
    """vc_adam: g = grad_scale g + wd p before the moments (torch.optim.Adam), n no multiple of 4 or of the block"""
    lr, b1, b2, eps, wd, gs, t0 = 5e-4, 0.9, 0.999, 1e-8, 5e-3, 0.5, 2.0
    p, g = uni(n, seed=1), uni(n, seed=2) * 0.1
    m, v = uni(n, seed=3) * 0.01, uni(n, seed=4, lo=0.0) * 1e-4
    hyper = torch.tensor([lr, b1, b2, eps, wd, gs], device=DEV)
    step = torch.tensor([t0, 0.0, 0.0], device=DEV)
    P_ = Guarded(1, n, init=p)
    M_, V_ = Guarded(1, n, init=m), Guarded(1, n, init=v)
    gd = g.to(DEV)
    L.vc_adam(n, P_.ptr, gd.data_ptr(), M_.ptr, V_.ptr, hyper.data_ptr(), step.data_ptr(), S())
    t = t0 + 1
    g64 = gs * g.double() + wd * p.double()
    m64 = b1 * m.double() + (1 - b1) * g64
    v64 = b2 * v.double() + (1 - b2) * g64 * g64
    p64 = p.double() - lr / (1 - b1 ** t) * m64 / (v64.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
    within("vc_adam p", n, rel_err(P_.check()[0], p64), 1e-6)
    within("vc_adam m", n, rel_err(M_.check()[0], m64), 1e-6)
    within("vc_adam v", n, rel_err(V_.check()[0], v64), 1e-6)
    assert float(step[0]) == t
    assert float((P_.check()[0].double() - p.double()).abs().max()) > 1e-5
