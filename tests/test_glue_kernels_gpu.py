"""Per-kernel parity of the fusion glue, the classifier head, AdamW and the small utilities of csrc/misc.hip,
and of the NCHW -> channels-last transposes of csrc/conv.hip, on the MI355X: each entry point against a CPU
reference written here (float64 where arithmetic is involved), at shapes the models never take: leading
dimensions above C, null gradient outputs, more than 96 pooled rows and more than 16 classes in the head,
C % 64 in {0, 1, 63}, the AdamW scalar tail with weight decay and a gradient scale, tiles that are no
multiple of 32 in the transposes.

Outputs start as NaN (or the accumulated-into values) and are followed by a guard region, gap columns
included (helpers.Guarded).  Copies are bit-exact; one add or fma: rel_err < 1e-6; the head: 1e-4 of the
reference's max |value|; AdamW: |param - float64 reference| <= 2e-6 after each of two steps at lr 8e-4.
"""
import pytest
import torch

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


def P(t):
    return t.data_ptr() if t is not None else None


def uni(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * 0.97130763   # off torch.rand's 2^-24 grid: sums round


def ints(*shape, seed=0):
    """integer-valued fp32 in [-8, 8]: sums of products of these are exact in float64"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).float()


def strided(t, ld, fill=3.5):
    rows, C = t.shape
    buf = torch.full((rows, ld), fill, device=DEV)
    buf[:, :C] = t.to(DEV)
    return buf


# ---------------------------------------------------------------------------------------------- cat2
CAT2 = [(50, 128, 128, 1, 128, 128), (7, 5, 5, 1, 8, 5), (7, 16, 3, 0, 16, 7), (7, 3, 16, 0, 3, 16)]


def cat2_ref(x1, x2, exchange):
    """torch.concat((x1, x2), 1) with the even channels of the two halves swapped when exchange"""
    a, b = x1.clone(), x2.clone()
    if exchange:
        a[:, 0::2], b[:, 0::2] = x2[:, 0::2], x1[:, 0::2]
    return torch.cat([a, b], 1)


@pytest.mark.parametrize("M,C1,C2,exchange,ld1,ld2", CAT2)
def test_cat2_fwd_bwd(L, M, C1, C2, exchange, ld1, ld2):
    x1, x2, dout = ints(M, C1, seed=1), ints(M, C2, seed=2), ints(M, C1 + C2, seed=3)
    x1d, x2d, dod = strided(x1, ld1), strided(x2, ld2), dout.to(DEV)
    out = Guarded(M, C1 + C2)
    assert L.vc_cat2_fwd(M, C1, C2, P(x1d), ld1, P(x2d), ld2, exchange, out.ptr, S()) == 0
    got = out.check()
    assert torch.equal(got, cat2_ref(x1, x2, exchange))
    # the gradient of that copy, from autograd of the reference
    a, b = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
    cat2_ref(a, b, exchange).backward(dout.double())
    g1, g2 = a.grad.float(), b.grad.float()
    dx1, dx2 = Guarded(M, C1, ld=ld1), Guarded(M, C2, ld=ld2)
    assert L.vc_cat2_bwd(M, C1, C2, P(dod), exchange, dx1.ptr, ld1, 0.0, dx2.ptr, ld2, 0.0, S()) == 0
    got1, got2 = dx1.check(), dx2.check()
    assert torch.equal(got1, g1) and torch.equal(got2, g2)
    # exact adjoint: <cat2(x1, x2), dout> = <x1, dx1> + <x2, dx2> (integer data: every sum exact)
    lhs = float((got.double() * dout.double()).sum())
    assert lhs == float((x1.double() * got1.double()).sum() + (x2.double() * got2.double()).sum())
    # one output null: the other is still written, nothing else is
    dx1 = Guarded(M, C1, ld=ld1)
    assert L.vc_cat2_bwd(M, C1, C2, P(dod), exchange, dx1.ptr, ld1, 0.0, None, ld2, 0.0, S()) == 0
    assert torch.equal(dx1.check(), g1)
    dx2 = Guarded(M, C2, ld=ld2)
    assert L.vc_cat2_bwd(M, C1, C2, P(dod), exchange, None, ld1, 0.0, dx2.ptr, ld2, 0.0, S()) == 0
    assert torch.equal(dx2.check(), g2)
    # beta 1: accumulate (one fma)
    p1, p2 = uni(M, C1, seed=4), uni(M, C2, seed=5)
    dn = uni(M, C1 + C2, seed=6)
    a, b = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
    cat2_ref(a, b, exchange).backward(dn.double())
    dnd = dn.to(DEV)
    dx1, dx2 = Guarded(M, C1, ld=ld1, init=p1), Guarded(M, C2, ld=ld2, init=p2)
    assert L.vc_cat2_bwd(M, C1, C2, P(dnd), exchange, dx1.ptr, ld1, 1.0, dx2.ptr, ld2, 1.0, S()) == 0
    shape = f"M={M},C1={C1},C2={C2},ex={exchange}"
    within("cat2_bwd beta=1 dx1", shape, rel_err(dx1.check().numpy(), (p1.double() + a.grad).numpy()), 1e-6)
    within("cat2_bwd beta=1 dx2", shape, rel_err(dx2.check().numpy(), (p2.double() + b.grad).numpy()), 1e-6)


# ---------------------------------------------------------------------------------------------- add2_2d
@pytest.mark.parametrize("use_b", [False, True])
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_add2_2d(L, use_b, beta):
    M, C, lda, ldb, ldo = 37, 19, 23, 19, 29
    a, b, o0 = uni(M, C, seed=7), uni(M, C, seed=8), uni(M, C, seed=9)
    ad, bd = strided(a, lda), strided(b, ldb)
    out = Guarded(M, C, ld=ldo, init=o0 if beta else None)
    assert L.vc_add2_2d(M, C, P(ad), lda, P(bd) if use_b else None, ldb, out.ptr, ldo, beta, S()) == 0
    ref = a.double() + (b.double() if use_b else 0.0) + (o0.double() if beta else 0.0)
    within("add2_2d", f"M={M},C={C},b={int(use_b)},beta={beta}", rel_err(out.check().numpy(), ref.numpy()), 1e-6)


# ---------------------------------------------------------------------------------------------- head
@pytest.mark.parametrize("B,S1,S2,C,ncls", [(4, 49, 25, 128, 16), (2, 1, 1, 1, 1), (3, 100, 97, 63, 17),
                                            (2, 81, 49, 127, 40), (5, 7, 130, 64, 7)])
def test_head_fwd_bwd(L, B, S1, S2, C, ncls):
    f1, f2 = uni(B, S1, C, seed=10), uni(B, S2, C, seed=11)
    W, bias, dlog = uni(ncls, C, seed=12), uni(ncls, seed=13), uni(B, ncls, seed=14)
    r = [t.double().requires_grad_(True) for t in (f1, f2, W, bias)]
    ref_feat = r[0].mean(1) + r[1].mean(1)
    ref_logits = ref_feat @ r[2].t() + r[3]
    ref_logits.backward(dlog.double())
    f1d, f2d, Wd, bd, dld = (t.to(DEV) for t in (f1, f2, W, bias, dlog))
    feat, logits = Guarded(B, C), Guarded(B, ncls)
    assert L.vc_head_fwd(B, S1, S2, C, ncls, P(f1d), P(f2d), P(Wd), P(bd), feat.ptr, logits.ptr, S()) == 0
    shape = f"B={B},S1={S1},S2={S2},C={C},ncls={ncls}"
    within("head_fwd.feat", shape, rel_err(feat.check().numpy(), ref_feat.detach().numpy()), 1e-4)
    within("head_fwd.logits", shape, rel_err(logits.check().numpy(), ref_logits.detach().numpy()), 1e-4)
    df1, df2, dW, db = Guarded(B * S1, C), Guarded(B * S2, C), Guarded(ncls, C), Guarded(1, ncls)
    assert L.vc_head_bwd(B, S1, S2, C, ncls, P(dld), P(Wd), feat.ptr, df1.ptr, df2.ptr, dW.ptr, db.ptr, S()) == 0
    within("head_bwd.df1", shape, rel_err(df1.check().numpy(), r[0].grad.view(B * S1, C).numpy()), 1e-4)
    within("head_bwd.df2", shape, rel_err(df2.check().numpy(), r[1].grad.view(B * S2, C).numpy()), 1e-4)
    within("head_bwd.dW", shape, rel_err(dW.check().numpy(), r[2].grad.numpy()), 1e-4)
    within("head_bwd.db", shape, rel_err(db.check()[0].numpy(), r[3].grad.numpy()), 1e-4)


# ---------------------------------------------------------------------------------------------- AdamW
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 7, 1027])
def test_adamw_two_steps(L, n, grad_scale):
    """the float4 body and the scalar tail (n % 4 != 0) with weight decay and a gradient scale, against a
    float64 AdamW written out here; the hyper-parameters are the fp32 values the kernel reads, widened"""
    hyper = torch.tensor([8e-4, 0.9, 0.999, 1e-8, 0.01, grad_scale], dtype=torch.float32)
    lr, b1, b2, eps, wd, gs = (float(v) for v in hyper.double())
    p0 = uni(n, seed=20)
    grads = [uni(n, seed=21), uni(n, seed=22)]
    p = Guarded(1, n, init=p0)
    m, v = Guarded(1, n, init=torch.zeros(n)), Guarded(1, n, init=torch.zeros(n))
    hd, step = hyper.to(DEV), torch.zeros(3, device=DEV)
    rp, rm, rv = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in (1, 2):
        g = Guarded(1, n, init=grads[t - 1])
        assert L.vc_adamw(n, p.ptr, g.ptr, m.ptr, v.ptr, P(hd), P(step), S()) == 0
        assert torch.equal(g.check()[0], grads[t - 1])
        bc1, sbc2 = 1.0 - b1 ** t, (1.0 - b2 ** t) ** 0.5
        st = step.cpu().double()
        assert float(st[0]) == float(t)
        assert abs(float(st[1]) - bc1) / bc1 < 1e-4 and abs(float(st[2]) - sbc2) / sbc2 < 1e-4
        gi = grads[t - 1].double() * gs
        rp = rp * (1.0 - lr * wd)
        rm = b1 * rm + (1.0 - b1) * gi
        rv = b2 * rv + (1.0 - b2) * gi * gi
        rp = rp - (lr / bc1) * rm / (rv.sqrt() / sbc2 + eps)
        shape = f"n={n},gs={grad_scale},step={t}"
        within("adamw.param", shape, float((p.check()[0].double() - rp).abs().max()), 2e-6, inclusive=True)
        within("adamw.exp_avg", shape, rel_err(m.check()[0].numpy(), rm.numpy()), 1e-5)
        within("adamw.exp_avg_sq", shape, rel_err(v.check()[0].numpy(), rv.numpy()), 1e-5)


# ---------------------------------------------------------------------------------------------- small utilities
def test_relu_bwd(L):
    n = 1000 + 3
    y, dy = uni(n, seed=30), uni(n, seed=31)
    y[:4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30])   # +-0 exactly: neither passes the gradient
    yd, dyd = y.to(DEV), dy.to(DEV)
    dx = Guarded(1, n)
    assert L.vc_relu_bwd(n, P(dyd), P(yd), dx.ptr, S()) == 0
    assert torch.equal(dx.check()[0], torch.where(y > 0, dy, torch.zeros(())))


def test_fill_and_fill_2d(L):
    n = 1000 + 3
    buf = Guarded(1, n)
    assert L.vc_fill(n, buf.ptr, 2.5, S()) == 0
    assert torch.equal(buf.check()[0], torch.full((n,), 2.5))
    for M, C, ld in [(37, 19, 29), (5, 64, 64), (300, 1, 3)]:
        buf = Guarded(M, C, ld=ld)
        assert L.vc_fill_2d(M, C, buf.ptr, ld, -1.5, S()) == 0
        assert torch.equal(buf.check(), torch.full((M, C), -1.5))


def test_fill_index_and_index_add(L):
    size, n = 1000, 300
    idx = torch.randperm(size, generator=torch.Generator().manual_seed(40))[:n].int()   # distinct
    base = uni(size, seed=41)
    buf = Guarded(1, size, init=base)
    idd = idx.to(DEV)
    assert L.vc_fill_index(n, P(idd), buf.ptr, 0.0, S()) == 0
    ref = base.clone()
    ref[idx.long()] = 0.0
    assert torch.equal(buf.check()[0], ref)
    cnt0 = torch.randint(0, 1 << 40, (size,), generator=torch.Generator().manual_seed(42))
    cnt = Guarded(1, size, init=cnt0, dtype=torch.int64)
    for _ in range(2):
        assert L.vc_index_add_i64(n, P(idd), cnt.ptr, 1, S()) == 0
    ref = cnt0.clone()
    ref[idx.long()] += 2
    assert torch.equal(cnt.check()[0], ref)


# ---------------------------------------------------------------------------------------------- NCHW -> NHWC
@pytest.mark.parametrize("B,C,HW,ldy", [(2, 144, 81, 144), (3, 1, 121, 1), (3, 1, 121, 4), (2, 33, 31, 33),
                                        (2, 33, 31, 40), (1, 63, 49, 63)])
def test_nchw_to_nhwc(L, B, C, HW, ldy):
    x = uni(B, C, HW, seed=50)
    xd = x.to(DEV)
    ref = x.permute(0, 2, 1).reshape(B * HW, C)
    if ldy == C:
        y = Guarded(B * HW, C)
        assert L.vc_nchw_to_nhwc(B, C, HW, P(xd), y.ptr, S()) == 0
        assert torch.equal(y.check(), ref)
    y = Guarded(B * HW, ldy)     # every column of the padded rows is written: C .. ldy - 1 with 0
    assert L.vc_nchw_to_nhwc_pad(B, C, HW, P(xd), y.ptr, ldy, S()) == 0
    got = y.check()
    assert torch.equal(got[:, :C], ref)
    assert bool((got[:, C:].view(torch.int32) == 0).all())
