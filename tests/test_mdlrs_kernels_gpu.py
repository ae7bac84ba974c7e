"""Per-kernel parity of csrc/mdlrs.hip on the MI355X: the padded max pool against torch's own MaxPool2d(2, 2, 1) on
the CPU (values, winning taps and the routed gradient bit for bit), the average-pool head and the cross-fusion loss
against float64 written here from the formulas in include/vitcnn.h.

Shapes are the smallest at which the kernels can go wrong: odd and even maps down to 2 x 2 (every output then has
padded taps), channel counts below, at and above a wave and no multiple of 4, padded leading dimensions, more than
one block (B H W C = 2 * 49 * 130 elements over 256-thread blocks).  Outputs start as NaN and are followed by a guard
region (helpers.Guarded) that must stay untouched; padded inputs carry NaN in their gap columns (helpers.Poisoned).
Tolerances: the pool is a selection, so bit-exact; head and loss 1e-5 of the reference's max |value| (sums of at most
a few hundred fp32 terms, 6e-8 each).
"""
import pytest
import torch
import torch.nn.functional as F

from helpers import Guarded, Poisoned, rel_err, within

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAPS = [(7, 7), (4, 4), (5, 5), (3, 3), (2, 2)]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vitcnn_amd._lib import lib
    return lib()


def S():
    return torch.cuda.current_stream().cuda_stream


def uni(*shape, seed=0, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def rows(t):
    """NCHW -> channels-last rows [B H W, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


# ---------------------------------------------------------------------------------------------- padded max pool
def torch_pool(x, dy):
    """torch's pool of x [B,C,H,W] on the CPU: y, the winning tap kh * 2 + kw per output, and the gradient for dy"""
    x = x.clone().requires_grad_(True)
    y, idx = F.max_pool2d(x, 2, 2, 1, return_indices=True)
    y.backward(dy)
    W = x.shape[3]
    OH, OW = y.shape[2:]
    ih, iw = idx // W, idx % W
    oh = torch.arange(OH).view(1, 1, OH, 1)
    ow = torch.arange(OW).view(1, 1, 1, OW)
    tap = (ih - (2 * oh - 1)) * 2 + (iw - (2 * ow - 1))
    assert int(tap.min()) >= 0 and int(tap.max()) <= 3
    return y.detach(), tap.to(torch.uint8), x.grad


def run_pool(L, x, dy, ldx, bn=None, relu_y=False):
    """the HIP pool of x [B,C,H,W] (rows of ld ldx) and its backward for dy: y, arg, dx as NCHW / rows"""
    B, C, H, W = x.shape
    OH, OW = H // 2 + 1, W // 2 + 1
    xin = Poisoned(rows(x), ld=ldx)
    y, arg = Guarded(B * OH * OW, C), Guarded(B * OH * OW, C, dtype=torch.uint8)
    ptrs = [t.data_ptr() for t in bn] if bn is not None else [None] * 4
    L.vc_maxpool2p_fwd(B, H, W, C, xin.ptr, ldx, *ptrs, y.ptr, arg.ptr, S())
    yv, av = y.check(), arg.check()
    dyd = rows(dy).to(DEV)
    yd = yv.to(DEV)
    dx = Guarded(B * H * W, C, ld=ldx)
    L.vc_maxpool2p_bwd(B, H, W, C, dyd.data_ptr(), arg.view.data_ptr(), yd.data_ptr() if relu_y else None, dx.ptr, ldx,
                       S())
    return yv, av, dx.check()


@pytest.mark.parametrize("pad", [0, 3], ids=["ld=C", "ld=C+3"])
@pytest.mark.parametrize("C", [5, 32, 130])
@pytest.mark.parametrize("H,W", MAPS)
def test_maxpool2p_matches_torch_bit_for_bit(L, H, W, C, pad):
    B = 2
    OH, OW = H // 2 + 1, W // 2 + 1
    x = uni(B, C, H, W, seed=H * 100 + C)
    dy = uni(B, C, OH, OW, seed=H * 100 + C + 1)
    y_ref, tap_ref, dx_ref = torch_pool(x, dy)
    y, arg, dx = run_pool(L, x, dy, C + pad)
    assert torch.equal(y, rows(y_ref))
    assert torch.equal(arg, rows(tap_ref))
    assert torch.equal(dx, rows(dx_ref))


@pytest.mark.parametrize("C", [5, 130])
@pytest.mark.parametrize("H,W", MAPS)
def test_maxpool2p_ties_and_all_negative_maps(L, H, W, C):
    """a post-ReLU-like map (>= 0, about half exact zeros: many windows tie, the first in-range tap must win) and an
    all-negative map (a padding of 0 instead of -inf would win every border window)"""
    B = 2
    OH, OW = H // 2 + 1, W // 2 + 1
    dy = uni(B, C, OH, OW, seed=7)
    tied = torch.relu(uni(B, C, H, W, seed=H + C))
    if H > 2:
        assert 0.3 < float((tied == 0).float().mean()) < 0.7
    neg = uni(B, C, H, W, seed=H + C + 1, lo=-2.0, hi=-0.5)
    for x in (tied, neg):
        y_ref, tap_ref, dx_ref = torch_pool(x, dy)
        y, arg, dx = run_pool(L, x, dy, C + 3)
        assert torch.equal(y, rows(y_ref)) and torch.equal(arg, rows(tap_ref)) and torch.equal(dx, rows(dx_ref))
    assert bool((rows(F.max_pool2d(neg, 2, 2, 1)) < 0).all())
    # with y: the ReLU mask y > 0 is folded in, dx is 0 wherever the pooled value is 0
    y, arg, dx = run_pool(L, tied, dy, C + 3, relu_y=True)
    y_ref, _, dx_ref = torch_pool(tied, dy * (F.max_pool2d(tied, 2, 2, 1) > 0))
    assert torch.equal(dx, rows(dx_ref))
    n_zero = int((y == 0).sum())
    assert n_zero > 0 or H == 2
    # every input pixel belongs to one window: the gradient that reaches dx is dy where y > 0, nothing else
    assert float(dx.abs().sum()) == pytest.approx(float((rows(dy) * (y > 0)).abs().sum()), rel=1e-5)


@pytest.mark.parametrize("C", [5, 32, 130])
@pytest.mark.parametrize("H,W", MAPS)
def test_maxpool2p_bn_fused_equals_bn_apply_relu_then_pool(L, H, W, C):
    """with the four BatchNorm pointers the pool sees relu((x - mean) * invstd * w + b): y bit-identical to the
    library's own vc_bn_apply (relu = 1) followed by the plain pool, the taps identical; some scales are negative, so
    pooling in front of the affine would pick other taps"""
    B = 2
    OH, OW = H // 2 + 1, W // 2 + 1
    M = B * H * W
    x = uni(B, C, H, W, seed=C + H, lo=-2.0, hi=2.0)
    mean, invstd = uni(C, seed=1, lo=-0.5, hi=0.5), uni(C, seed=2, lo=0.5, hi=2.0)
    w, b = uni(C, seed=3, lo=0.2, hi=1.5), uni(C, seed=4, lo=-0.3, hi=0.3)
    w[::2] = -w[::2]          # every other channel has a negative scale
    assert bool((w < 0).any()) and bool((w > 0).any())
    bn = [t.to(DEV) for t in (mean, invstd, w, b)]
    xd = rows(x).to(DEV)
    z = Guarded(M, C)
    L.vc_bn_apply(M, C, xd.data_ptr(), C, *[t.data_ptr() for t in bn], 1, z.ptr, C, S())
    zv = z.check()
    z_nchw = zv.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()
    dy = uni(B, C, OH, OW, seed=9)
    y_plain, arg_plain, _ = run_pool(L, z_nchw, dy, C)
    y_fused, arg_fused, dx = run_pool(L, x, dy, C + 3, bn=bn, relu_y=True)
    assert torch.equal(y_fused, y_plain) and torch.equal(arg_fused, arg_plain)
    # against torch on the library's post-BN map: values, taps, and the gradient with the ReLU mask folded in
    y_ref, tap_ref, dx_ref = torch_pool(z_nchw, dy * (F.max_pool2d(z_nchw, 2, 2, 1) > 0))
    assert torch.equal(y_fused, rows(y_ref)) and torch.equal(arg_fused, rows(tap_ref))
    assert torch.equal(dx, rows(dx_ref))
    assert bool((dx[(rows(torch_unpool_mask(y_fused, B, C, H, W)) == 0)] == 0).all())
    # and against the formula in float64
    ref64 = torch.relu((x.double() - mean.double().view(1, C, 1, 1)) * invstd.double().view(1, C, 1, 1)
                       * w.double().view(1, C, 1, 1) + b.double().view(1, C, 1, 1))
    within("vc_maxpool2p_fwd bn", (H, W, C), rel_err(y_fused, rows(F.max_pool2d(ref64, 2, 2, 1))), 1e-5)


def torch_unpool_mask(y_rows, B, C, H, W):
    """per input pixel, the pooled value of the window it belongs to (NCHW)"""
    OH, OW = H // 2 + 1, W // 2 + 1
    y = y_rows.reshape(B, OH, OW, C).permute(0, 3, 1, 2)
    hh = (torch.arange(H) + 1) // 2
    ww = (torch.arange(W) + 1) // 2
    return y[:, :, hh][:, :, :, ww].contiguous()


# ---------------------------------------------------------------------------------------------- average-pool head
@pytest.mark.parametrize("G,mode", [(1, 0), (2, 0), (3, 1)], ids=["G1", "G2-concat", "G3-separate"])
@pytest.mark.parametrize("ncls", [7, 16])
@pytest.mark.parametrize("C", [64, 6])
@pytest.mark.parametrize("HW", [4, 9, 16])
@pytest.mark.parametrize("B", [1, 3])
def test_avgpool_head_fwd_bwd(L, B, HW, C, ncls, G, mode):
    Cin = C if mode else G * C
    R = G * B if mode else B
    maps = [uni(B, HW, C, seed=10 * g + HW) for g in range(G)]
    Wt, bias = uni(ncls, Cin, seed=40), uni(ncls, seed=41)
    dlog = uni(R, ncls, seed=42)
    m64 = [m.double().requires_grad_(True) for m in maps]
    W64, b64 = Wt.double().requires_grad_(True), bias.double().requires_grad_(True)
    pooled64 = [m.mean(1) for m in m64]                                         # [B, C] each
    op64 = torch.cat(pooled64, 0) if mode else torch.cat(pooled64, 1)           # [R, Cin]
    logits64 = op64 @ W64.t() + b64
    logits64.backward(dlog.double())
    md = [m.to(DEV).contiguous() for m in maps]
    f = [m.data_ptr() for m in md] + [None] * (3 - G)
    Wd, bd, dld = Wt.to(DEV), bias.to(DEV), dlog.to(DEV)

    def run():
        pooled, logits = Guarded(R, Cin), Guarded(R, ncls)
        L.vc_avgpool_head_fwd(B, HW, C, G, ncls, mode, f[0], f[1], f[2], Wd.data_ptr(), bd.data_ptr(), pooled.ptr,
                              logits.ptr, S())
        pv, lv = pooled.check(), logits.check()
        dfs = [Guarded(B * HW, C) for _ in range(G)]
        d = [t.ptr for t in dfs] + [None] * (3 - G)
        dW, db = Guarded(ncls, Cin), Guarded(1, ncls)
        L.vc_avgpool_head_bwd(B, HW, C, G, ncls, mode, dld.data_ptr(), Wd.data_ptr(), pooled.view.data_ptr(), d[0], d[1],
                              d[2], dW.ptr, db.ptr, S())
        return pv, lv, [t.check() for t in dfs], dW.check(), db.check()[0]

    pv, lv, dfs, dW, db = run()
    shape = (B, HW, C, ncls, G, mode)
    within("vc_avgpool_head_fwd pooled", shape, rel_err(pv, op64.detach()), 1e-5)
    within("vc_avgpool_head_fwd logits", shape, rel_err(lv, logits64.detach()), 1e-5)
    within("vc_avgpool_head_bwd dW", shape, rel_err(dW, W64.grad), 1e-5)
    within("vc_avgpool_head_bwd db", shape, rel_err(db, b64.grad), 1e-5)
    for g in range(G):
        within(f"vc_avgpool_head_bwd df{g}", shape, rel_err(dfs[g], m64[g].grad.reshape(B * HW, C)), 1e-5)
    # the sums run in a fixed order: a second call gives the same bits
    pv2, lv2, dfs2, dW2, db2 = run()
    assert torch.equal(pv, pv2) and torch.equal(lv, lv2) and torch.equal(dW, dW2) and torch.equal(db, db2)
    assert all(torch.equal(a, b) for a, b in zip(dfs, dfs2))


# ---------------------------------------------------------------------------------------------- cross-fusion loss
def loss_inputs(B, ncls):
    o = [uni(B, ncls, seed=50 + i, lo=-3.0, hi=3.0) for i in range(3)]
    g = torch.Generator().manual_seed(B + ncls)
    target = torch.randint(1, ncls, (B,), generator=g)
    if B >= 4:
        target[1::4] = 0          # class 0 carries weight 0: these samples drop out of the cross entropy
    weight = uni(ncls, seed=60, lo=0.5, hi=1.5)
    weight[0] = 0.0
    return o, target, weight


def run_loss(L, o, target, weight):
    B, ncls = o[0].shape
    od = [t.to(DEV).contiguous() for t in o]
    td, wd = target.to(DEV), weight.to(DEV)
    loss = Guarded(1, 1)
    d = [Guarded(B, ncls) for _ in range(3)]
    L.vc_xfusion_loss_fwd_bwd(B, ncls, od[0].data_ptr(), od[1].data_ptr(), od[2].data_ptr(), td.data_ptr(),
                              wd.data_ptr(), loss.ptr, d[0].ptr, d[1].ptr, d[2].ptr, S())
    return loss.check()[0, 0], [t.check() for t in d]


@pytest.mark.parametrize("ncls", [12, 16])
@pytest.mark.parametrize("B", [1, 4, 64])
def test_xfusion_loss_fwd_bwd(L, B, ncls):
    o, target, weight = loss_inputs(B, ncls)
    o64 = [t.double().requires_grad_(True) for t in o]
    ref = F.cross_entropy(o64[0], target, weight=weight.double()) + ((o64[0] - o64[1]) ** 2).mean() \
        + ((o64[0] - o64[2]) ** 2).mean()
    ref.backward()
    loss, d = run_loss(L, o, target, weight)
    within("vc_xfusion_loss_fwd_bwd loss", (B, ncls), abs(float(loss) - float(ref)) / abs(float(ref)), 1e-5)
    for i in range(3):
        within(f"vc_xfusion_loss_fwd_bwd do{i + 1}", (B, ncls), rel_err(d[i], o64[i].grad), 1e-5)


@pytest.mark.parametrize("ncls", [12, 16])
@pytest.mark.parametrize("B", [1, 4, 64])
def test_xfusion_loss_with_equal_outputs_is_the_cross_entropy(L, B, ncls):
    """o2 = o3 = o1: both squared differences vanish, the loss and do1 are vc_ce_fwd_bwd's, do2 = do3 = 0 exactly"""
    o, target, weight = loss_inputs(B, ncls)
    loss, d = run_loss(L, [o[0], o[0], o[0]], target, weight)
    od, td, wd = o[0].to(DEV).contiguous(), target.to(DEV), weight.to(DEV)
    ce, dce = Guarded(1, 1), Guarded(B, ncls)
    L.vc_ce_fwd_bwd(B, ncls, od.data_ptr(), td.data_ptr(), wd.data_ptr(), -100, ce.ptr, dce.ptr, S())
    assert torch.equal(loss, ce.check()[0, 0])
    assert torch.equal(d[0], dce.check())
    assert bool((d[1] == 0).all()) and bool((d[2] == 0).all())
