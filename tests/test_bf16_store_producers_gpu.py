"""The producers of the stored bf16 operands: vc_cast_bf16_2d against torch's own RNE
`Tensor.bfloat16()`, bit for bit; vc_conv3x3_pack_bf16_many against the cast of the fp32 arena; and the BatchNorm
kernels' extra bf16 outputs (vc_bn_forward_ex_h, vc_bn_bwd_relu_ex_h) against the cast of the fp32 output they keep
writing, with the fp32 outputs and statistics bit-equal to the plain entry points'."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0x5A5A   # what the bytes around a bf16 output hold before the call


def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vitcnn_amd._lib import lib
    return lib(), torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.bfloat16().view(torch.int16)


def _specials():
    """exact ties (to even: down and up), both signs; +-0; +-inf; values that round up into the next binade"""
    pos = [0x3F808000, 0x3F818000, 0x42FE8000, 0x42FF8000,   # ties: 1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6, ...
           0x00000000, 0x7F800000,                           # 0, inf
           0x3FFFFFFF, 0x3FFF8000, 0x40FFC000,               # -> 2.0 (all ones; a tie; above the tie)
           0x3F808001, 0x3F807FFF]                           # one ulp either side of a tie
    bits = pos + [b | 0x80000000 for b in pos]
    return torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in bits], dtype=torch.int32).view(torch.float32)


@pytest.mark.parametrize("M,C,ldd", [(3, 5, 8), (130, 2193, 2200)])
def test_cast_is_torch_rne_bit_for_bit(M, C, ldd):
    L, s = _lib()
    g = torch.Generator().manual_seed(M + C)
    src = torch.randn(M, C, generator=g)
    sp = _specials()
    if M * C >= sp.numel():
        src.view(-1)[:sp.numel()] = sp
    else:   # the small shape: as many specials as fit, ties and zeros first
        src.view(-1)[:] = sp[torch.arange(M * C) % sp.numel()]
    lds = C + 3
    src_d = torch.full((M, lds), float("nan"), device=DEV)
    src_d[:, :C] = src.to(DEV)
    dst = torch.full((M * ldd + 64,), SENT, dtype=torch.int16, device=DEV)
    L.vc_cast_bf16_2d(M, C, src_d.data_ptr(), lds, dst.data_ptr(), ldd, s)
    torch.cuda.synchronize()
    out = dst.cpu()
    rows = out[:M * ldd].view(M, ldd)
    assert torch.equal(rows[:, :C], _bits(src))
    assert bool((rows[:, C:] == 0).all()), "pad columns"
    assert bool((out[M * ldd:] == SENT).all()), "store past the last row"


def test_cast_of_all_specials():
    """every special value, whatever the shapes above kept of them"""
    L, s = _lib()
    sp = _specials()
    n = sp.numel()
    dst = torch.full((_up8(n) + 64,), SENT, dtype=torch.int16, device=DEV)
    L.vc_cast_bf16_2d(1, n, sp.to(DEV).data_ptr(), n, dst.data_ptr(), _up8(n), s)
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu()[:n], _bits(sp))


def _up8(n):
    return (n + 7) // 8 * 8


def test_packed_bf16_arena_is_the_cast_of_the_fp32_arena():
    L, s = _lib()
    shapes = [(50, 37), (16, 1), (4, 2193)]
    g = torch.Generator().manual_seed(5)
    ws = [torch.randn(O, C, 3, 3, generator=g).to(DEV) for O, C in shapes]
    n = len(shapes)
    a32 = [torch.full((O * 9 * ((C + 3) // 4 * 4),), float("nan"), device=DEV) for O, C in shapes]
    sizes = [O * 9 * _up8(C) for O, C in shapes]
    arena = torch.full((sum(sizes) + 64,), SENT, dtype=torch.int16, device=DEV)
    sh = (ctypes.c_int * (2 * n))(*[v for oc in shapes for v in oc])
    src = (ctypes.c_void_p * n)(*[w.data_ptr() for w in ws])
    d32 = (ctypes.c_void_p * n)(*[a.data_ptr() for a in a32])
    d16 = (ctypes.c_void_p * n)()
    off = 0
    for i, k in enumerate(sizes):
        d16[i] = arena.data_ptr() + 2 * off
        off += k
    L.vc_conv3x3_pack_many(n, ctypes.addressof(sh), ctypes.addressof(src), ctypes.addressof(d32), s)
    L.vc_conv3x3_pack_bf16_many(n, ctypes.addressof(sh), ctypes.addressof(src), ctypes.addressof(d16), s)
    torch.cuda.synchronize()
    out, off = arena.cpu(), 0
    for (O, C), a, k in zip(shapes, a32, sizes):
        got = out[off:off + k].view(O, 9, _up8(C))
        want = a.cpu().view(O, 9, (C + 3) // 4 * 4)[:, :, :C]
        assert torch.equal(got[:, :, :C], _bits(want)), (O, C)
        assert bool((got[:, :, C:] == 0).all()), (O, C)
        off += k
    assert bool((out[off:] == SENT).all()), "store behind the arena"


@pytest.mark.parametrize("train", [1, 0])
@pytest.mark.parametrize("M,C,pad16", [(242, 64, 0), (9, 1024, 8)])
def test_batchnorm_bf16_outputs_are_the_cast_of_the_fp32_outputs(train, M, C, pad16):
    """forward and backward through the ReLU; ld16 = C + pad16 (the pad columns are written zero)"""
    L, s = _lib()
    from vitcnn_amd.model import N_COUNTERS
    g = torch.Generator().manual_seed(M + C + train)
    x = torch.randn(M, C, generator=g).to(DEV)
    dy = torch.randn(M, C, generator=g).to(DEV)
    w, b = (torch.rand(C, generator=g) + 0.5).to(DEV), (0.3 * torch.randn(C, generator=g)).to(DEV)
    rm0, rv0 = torch.randn(C, generator=g).to(DEV), (torch.rand(C, generator=g) + 0.5).to(DEV)
    ws = torch.empty(1 << 20, device=DEV)
    cnt = torch.zeros(N_COUNTERS, dtype=torch.int32, device=DEV)
    ld16 = C + pad16
    res = []
    for half in (False, True):
        rm, rv = rm0.clone(), rv0.clone()
        mean, invstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        y, dx = torch.full((M, C), float("nan"), device=DEV), torch.full((M, C), float("nan"), device=DEV)
        dw, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        y16 = torch.full((M * ld16 + 64,), SENT, dtype=torch.int16, device=DEV)
        dx16 = torch.full((M * ld16 + 64,), SENT, dtype=torch.int16, device=DEV)
        fa = (train, M, C, x.data_ptr(), C, 1e-5, 0.1, mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(),
              rv.data_ptr(), w.data_ptr(), b.data_ptr(), 1, y.data_ptr(), C)
        ba = (train, M, C, dy.data_ptr(), C, x.data_ptr(), C, mean.data_ptr(), invstd.data_ptr(), w.data_ptr(),
              b.data_ptr(), dx.data_ptr(), C, 0.0)
        tail = (ws.data_ptr(), ws.numel(), cnt.data_ptr(), N_COUNTERS, s)
        if half:
            L.vc_bn_forward_ex_h(*fa, y16.data_ptr(), ld16, *tail)
            L.vc_bn_bwd_relu_ex_h(*ba, dx16.data_ptr(), ld16, dw.data_ptr(), db.data_ptr(), 0.0, *tail)
        else:
            L.vc_bn_forward_ex(*fa, *tail)
            L.vc_bn_bwd_relu_ex(*ba, dw.data_ptr(), db.data_ptr(), 0.0, *tail)
        torch.cuda.synchronize()
        assert int(cnt.abs().sum()) == 0
        res.append([t.cpu() for t in (y, mean, invstd, rm, rv, dx, dw, db, y16, dx16)])
    plain, h = res
    for i, name in enumerate(("y", "mean", "invstd", "running_mean", "running_var", "dx", "dw", "db")):
        assert torch.equal(plain[i], h[i]), name
    assert float(plain[0].min()) == 0.0 and bool(torch.isfinite(plain[5]).all())
    for f32, o16, name in ((h[0], h[8], "y16"), (h[5], h[9], "dx16")):
        rows = o16[:M * ld16].view(M, ld16)
        assert torch.equal(rows[:, :C], _bits(f32)), name
        assert bool((rows[:, C:] == 0).all()), name + " pad columns"
        assert bool((o16[M * ld16:] == SENT).all()), name + " tail"
    for o16 in (plain[8], plain[9]):   # the plain entry points know nothing of them
        assert bool((o16 == SENT).all())
