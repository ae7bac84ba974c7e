"""Per-kernel parity of csrc/fusatnet.hip on the MI355X: each entry point against a CPU reference written here
(torch unfold / fold, float64 autograd), at shapes FusAtNet itself never takes: H != W, leading dimensions
above C, col2im without accumulation, the scalar elementwise kernel next to the float4 one, pool sizes that
are no multiple of the 64-channel / 64-pixel blocking.

Outputs start as NaN (or the accumulated-into values) and are followed by a guard region, gap columns
included (helpers.Guarded).  Copies and single products are bit-exact; the nine-term col2im gather:
rel_err < 1e-6; pool_scale and its backward: 1e-4 of the reference's max |value|.
"""
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


def P(t):
    return t.data_ptr() if t is not None else None


def uni(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * 0.97130763   # off torch.rand's 2^-24 grid: sums round


def strided(t, ld, fill=3.5):
    """device copy of the rows of t [rows, C] at leading dimension ld (gap columns hold `fill`, never read)"""
    rows, C = t.shape
    buf = torch.full((rows, ld), fill, device=DEV)
    buf[:, :C] = t.to(DEV)
    return buf


# ---------------------------------------------------------------------------------------------- im2col / col2im
@pytest.mark.parametrize("B,H,W,C,pad,ld", [(2, 3, 3, 1, 0, 1), (2, 3, 5, 5, 1, 8), (1, 11, 11, 4, 1, 4),
                                            (3, 7, 6, 33, 0, 40)])
def test_im2col_col2im_pad(L, B, H, W, C, pad, ld):
    OH, OW = H + 2 * pad - 2, W + 2 * pad - 2
    x = uni(B * H * W, C, seed=1)
    xd = strided(x, ld)
    col = Guarded(B * OH * OW, 9 * C)
    assert L.vc_im2col3x3_pad(B, H, W, C, pad, P(xd), ld, col.ptr, S()) == 0
    nchw = x.view(B, H, W, C).permute(0, 3, 1, 2)
    ref_col = F.unfold(nchw, 3, padding=pad).permute(0, 2, 1).reshape(B * OH * OW, 9 * C)
    assert torch.equal(col.check(), ref_col)
    dcol, dx0 = uni(B * OH * OW, 9 * C, seed=2), uni(B * H * W, C, seed=3)
    dcd = dcol.to(DEV)
    fold = F.fold(dcol.double().view(B, OH * OW, 9 * C).permute(0, 2, 1), (H, W), 3, padding=pad)
    fold = fold.permute(0, 2, 3, 1).reshape(B * H * W, C)
    for accumulate in (0, 1):
        dx = Guarded(B * H * W, C, ld=ld, init=dx0 if accumulate else None)
        assert L.vc_col2im3x3_pad(B, H, W, C, pad, P(dcd), dx.ptr, ld, accumulate, S()) == 0
        ref = fold + dx0.double() if accumulate else fold
        within("col2im3x3_pad", f"B={B},H={H},W={W},C={C},pad={pad},ld={ld},acc={accumulate}",
               rel_err(dx.check().numpy(), ref.numpy()), 1e-6)


# ---------------------------------------------------------------------------------------------- mul2_2d
@pytest.mark.parametrize("M,C,lda,ldb,ldo,lead", [(37, 64, 64, 64, 64, 0),    # the float4 kernel
                                                  (37, 63, 63, 63, 63, 0),    # C % 4 != 0: scalar
                                                  (37, 64, 64, 64, 66, 0),    # ldo % 4 != 0: scalar
                                                  (37, 64, 64, 64, 64, 1),    # out one float off 16 B: scalar
                                                  (37, 64, 68, 72, 76, 0)])   # float4 with gaps in every operand
def test_mul2_2d(L, M, C, lda, ldb, ldo, lead):
    a, b = uni(M, 64, seed=4)[:, :C].contiguous(), uni(M, 64, seed=5)[:, :C].contiguous()
    ad, bd = strided(a, lda), strided(b, ldb)
    out = Guarded(M, C, ld=ldo, lead=lead)
    assert (out.ptr % 16 == 0) == (lead == 0)
    assert L.vc_mul2_2d(M, C, P(ad), lda, P(bd), ldb, out.ptr, ldo, S()) == 0
    assert torch.equal(out.check(), a * b)


def test_mul2_2d_scalar_on_misaligned_input(L):
    """an input base one float off 16 B also takes the scalar kernel (a float4 load there would fault or
    read the wrong four floats)"""
    M, C = 37, 64
    a, b = uni(M, C, seed=4), uni(M, C, seed=5)
    abuf = torch.zeros(M * C + 1, device=DEV)
    abuf[1:] = a.flatten().to(DEV)
    bd = b.to(DEV)
    out = Guarded(M, C)
    assert L.vc_mul2_2d(M, C, P(abuf) + 4, C, P(bd), C, out.ptr, C, S()) == 0
    assert torch.equal(out.check(), a * b)


# ---------------------------------------------------------------------------------------------- pool_scale
@pytest.mark.parametrize("B,HW,HWp,C,ldf,ldo,lddf", [(2, 121, 25, 1024, 1024, 1024, 1024), (3, 5, 1, 70, 72, 75, 80),
                                                     (1, 64, 4, 64, 64, 64, 64)])
def test_pool_scale_fwd_bwd(L, B, HW, HWp, C, ldf, ldo, lddf):
    pooled, Fm = uni(B, HWp, C, seed=6), uni(B, HW, C, seed=7)
    dout, dF0 = uni(B, HW, C, seed=8), uni(B, HW, C, seed=9)
    p64, f64 = pooled.double().requires_grad_(True), Fm.double().requires_grad_(True)
    ref = p64.mean(1, keepdim=True) * f64
    ref.backward(dout.double())
    pd, fd = pooled.to(DEV), strided(Fm.view(B * HW, C), ldf)
    out = Guarded(B * HW, C, ld=ldo)
    assert L.vc_pool_scale(B, HW, HWp, C, P(pd), P(fd), ldf, out.ptr, ldo, S()) == 0
    shape = f"B={B},HW={HW},HWp={HWp},C={C}"
    within("pool_scale", shape, rel_err(out.check().numpy(), ref.detach().view(B * HW, C).numpy()), 1e-4)
    # backward: dF accumulated into, dpooled overwritten; dout rows at their own leading dimension
    lddo = ldo
    dod = strided(dout.view(B * HW, C), lddo)
    dF = Guarded(B * HW, C, ld=lddf, init=dF0)
    dpooled = Guarded(B * HWp, C)
    assert L.vc_pool_scale_bwd(B, HW, HWp, C, P(pd), P(fd), ldf, P(dod), lddo, dF.ptr, lddf, dpooled.ptr, S()) == 0
    ref_dF = (dF0.double() + f64.grad).view(B * HW, C)
    within("pool_scale_bwd.dF", shape, rel_err(dF.check().numpy(), ref_dF.numpy()), 1e-4)
    within("pool_scale_bwd.dpooled", shape, rel_err(dpooled.check().numpy(), p64.grad.view(B * HWp, C).numpy()), 1e-4)
