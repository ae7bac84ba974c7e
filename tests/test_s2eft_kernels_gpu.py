"""Per-kernel parity of csrc/s2eft.hip on the MI355X: each entry point against a float64 CPU reference written
here from the formulas in include/vitcnn.h, at shapes the S2EFT model itself never takes (the C > 256 gate
tail, T < 16 and T = 256 attention, other head counts, the chunked attention grids).

Outputs start as NaN and are followed by a guard region (helpers.Guarded) that must stay untouched.
Copy / select kernels are bit-exact; one add or fma: rel_err < 1e-6; reductions and attention: 1e-4 of the
reference's max |value|; GELU: 4x torch's own fp32 deviation from float64 + 2 eps32 max|ref|.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import Guarded, rel_err, within

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vitcnn_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def probe():
    """libvitcnn_probe.so: the same kernels with the measurement knobs read from VITCNN_*"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vitcnn_amd._lib import probe_lib
    return probe_lib()


def S():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return t.data_ptr() if t is not None else None


def uni(*shape, seed=0, lo=-1.0, hi=1.0, scale=0.97130763):
    """uniform in [lo, hi) * scale; the default scale moves the values off torch.rand's 2^-24 grid, on which
    sums of two would be exact"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * (hi - lo) + lo) * scale


# ---------------------------------------------------------------------------------------------- spectral gate
GATE_BETA = 0.4
GATE_SHAPES = [(3, 145, 147), (2, 1, 5), (3, 5, 1), (2, 6, 300), (2, 7, 64), (2, 33, 257), (2, 200, 3), (2, 8, 256)]


def gate_case(B, N, C, seed):
    """x in [0, 1), conv weight in [-2, 2], and the bias that puts logit(beta) into the widest gap among the
    central half of the sorted float64 pre-activations: a mixed mask with every token away from the threshold"""
    x = uni(B, N, C, seed=seed, lo=0.0, hi=1.0, scale=1.0)
    w = uni(1, 2, 7, seed=seed + 100, lo=-2.0, hi=2.0, scale=1.0)
    xd = x.double()
    stats = torch.stack([xd.mean(2), xd.amax(2)], 1)           # [B, 2, N]
    pre = F.conv1d(stats, w.double(), padding=3)[:, 0]         # [B, N], no bias
    s = pre.flatten().sort().values
    n = s.numel()
    mid = s[n // 4:n - n // 4]
    if mid.numel() >= 2:
        gaps = mid[1:] - mid[:-1]
        i = int(gaps.argmax())
        cut = float((mid[i] + mid[i + 1]) / 2)
    else:
        cut = float(s[0]) - 1.0
    bias = torch.tensor([math.log(GATE_BETA / (1 - GATE_BETA)) - cut], dtype=torch.float32)
    sig = torch.sigmoid(pre + bias.double())
    return x, w, bias, sig


@pytest.mark.parametrize("B,N,C", GATE_SHAPES)
def test_gate_fwd(L, B, N, C):
    x, w, bias, sig = gate_case(B, N, C, seed=0)
    beta = float(np.float32(GATE_BETA))
    ref_mask = (sig >= beta).float()
    if B * N > 1:
        assert 0 < int(ref_mask.sum()) < B * N, "the reference mask must hold both values"
    margin = float((sig - beta).abs().min())
    assert margin > 1e-4, f"a reference sigmoid lies within 1e-4 of beta ({margin:.2e})"
    xg, mask = Guarded(B * N, C), Guarded(B, N)
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    assert L.vc_s2eft_gate_fwd(B, N, C, P(xd), P(wd), P(bd), GATE_BETA, xg.ptr, mask.ptr, S()) == 0
    got_mask, got_xg = mask.check(), xg.check()
    assert torch.equal(got_mask, ref_mask)
    assert torch.equal(got_xg, (x * ref_mask[:, :, None]).view(B * N, C))


# ---------------------------------------------------------------------------------------------- attention
ATT_SCALE = 0.25
ATT_T = [1, 2, 15, 16, 17, 31, 32, 33, 146, 255, 256]
ATT_BH = [(1, 1), (2, 3), (3, 4)]
ATT_REGIMES = ["uniform", "peaked", "peaked_last"]


def attn_inputs(B, T, H, regime, seed):
    """qkv [B*T, 3*H*16] (q | k | v column blocks) and dout [B*T, H*16], fp32"""
    g = torch.Generator().manual_seed(seed)
    if regime == "uniform":
        q = torch.rand(B, T, H, 16, generator=g) * 4 - 2
        k = torch.rand(B, T, H, 16, generator=g) * 4 - 2
    elif regime == "peaked":      # integer q, k: scores exact in fp32, spanning ~60 nats at scale 0.25
        q = torch.randint(-4, 5, (B, T, H, 16), generator=g).float()
        k = torch.randint(-4, 5, (B, T, H, 16), generator=g).float()
    else:                         # every query's largest score at the last key (the partial last tile)
        q = torch.randint(1, 5, (B, T, H, 16), generator=g).float()
        k = torch.randint(-4, 1, (B, T, H, 16), generator=g).float()
        k[:, T - 1] = 4.0
    v = torch.rand(B, T, H, 16, generator=g) * 2 - 1
    dout = torch.rand(B * T, H * 16, generator=g) * 2 - 1
    qkv = torch.stack([q, k, v], 2).reshape(B * T, 3 * H * 16).contiguous()
    return qkv, dout


def attn_reference(qkv, dout, B, T, H):
    x = qkv.double().requires_grad_(True)
    q, k, v = x.view(B, T, 3, H, 16).permute(2, 0, 3, 1, 4)          # [B, H, T, 16] each
    s = q @ k.transpose(-1, -2) * ATT_SCALE
    lse = torch.logsumexp(s, -1)                                     # [B, H, T]
    out = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B * T, H * 16)
    out.backward(dout.double())
    return out.detach(), lse.detach(), x.grad


def attn_run(lib, qkv, dout, B, T, H):
    qd, dd = qkv.to(DEV), dout.to(DEV)
    out, lse, dqkv = Guarded(B * T, H * 16), Guarded(B * H, T), Guarded(B * T, 3 * H * 16)
    assert lib.vc_s2eft_attn_fwd(B, T, H, P(qd), ATT_SCALE, out.ptr, lse.ptr, S()) == 0
    got_out, got_lse = out.check(), lse.check()
    # the backward is fed the kernel's own out and lse
    assert lib.vc_s2eft_attn_bwd(B, T, H, P(qd), out.ptr, P(dd), lse.ptr, ATT_SCALE, dqkv.ptr, S()) == 0
    return got_out, got_lse, dqkv.check()


@pytest.mark.parametrize("B,H", ATT_BH)
@pytest.mark.parametrize("T", ATT_T)
def test_attn_fwd_bwd(L, T, B, H):
    if T >= 255:
        B = 1
    for regime in ATT_REGIMES:
        qkv, dout = attn_inputs(B, T, H, regime, seed=T * 7 + H)
        ref_out, ref_lse, ref_dqkv = attn_reference(qkv, dout, B, T, H)
        if regime == "peaked_last" and T > 1:
            s = torch.einsum("bthd,bshd->bhts", *qkv.double().view(B, T, 3, H, 16).unbind(2)[:2])
            assert bool((s.argmax(-1) == T - 1).all())
        if T == 1:   # a single key: softmax is 1, dq and dk vanish
            assert float(ref_dqkv[:, :2 * H * 16].abs().max()) == 0.0
        out, lse, dqkv = attn_run(L, qkv, dout, B, T, H)
        shape = f"T={T},B={B},H={H},{regime}"
        within("attn_fwd.out", shape, rel_err(out.numpy(), ref_out.numpy()), 1e-4)
        within("attn_fwd.lse", shape, rel_err(lse.numpy(), ref_lse.view(B * H, T).numpy()), 1e-4)
        within("attn_bwd.dqkv", shape, rel_err(dqkv.numpy(), ref_dqkv.numpy()), 1e-4)


@pytest.mark.parametrize("T", [33, 146, 256])
def test_attn_chunked_grids_are_bit_identical(probe, T, monkeypatch):
    """the multi-chunk forward grid (wpb < waves; the product build never launches it) and the backward's
    chunkings give the default launch's bits"""
    B, H = 2, 3
    waves = (T + 15) // 16
    qkv, dout = attn_inputs(B, T, H, "uniform", seed=T)
    monkeypatch.delenv("VITCNN_ATTN_FWD_WPB", raising=False)
    monkeypatch.delenv("VITCNN_ATTN_BWD_WPB", raising=False)
    base = attn_run(probe, qkv, dout, B, T, H)
    ref_out, ref_lse, ref_dqkv = attn_reference(qkv, dout, B, T, H)
    assert rel_err(base[0].numpy(), ref_out.numpy()) < 1e-4 and rel_err(base[2].numpy(), ref_dqkv.numpy()) < 1e-4
    for fw in (1, 3, waves):
        for bw in (1, waves):
            monkeypatch.setenv("VITCNN_ATTN_FWD_WPB", str(fw))
            monkeypatch.setenv("VITCNN_ATTN_BWD_WPB", str(bw))
            got = attn_run(probe, qkv, dout, B, T, H)
            for a, b in zip(got, base):
                assert torch.equal(a, b), (fw, bw)


# ---------------------------------------------------------------------------------------------- GELU
def gelu_points():
    x = torch.cat([torch.linspace(-8, 8, 4097), torch.tensor([0.0, -0.0, 1e-8, -1e-8, 20.0, -20.0])])
    assert x.numel() == 4097 + 6 and x.numel() % 256 != 0
    return x


def test_gelu_fwd_bwd(L):
    x = gelu_points()
    n = x.numel()
    dy = uni(n, seed=5)
    x64 = x.double().requires_grad_(True)
    y64 = F.gelu(x64)
    y64.backward(dy.double())
    x32 = x.clone().requires_grad_(True)
    y32 = F.gelu(x32)
    y32.backward(dy)
    ref_y, ref_dx = y64.detach(), x64.grad
    torch_dev_y = float((y32.detach().double() - ref_y).abs().max())
    torch_dev_dx = float((x32.grad.double() - ref_dx).abs().max())
    xd, dyd = x.to(DEV), dy.to(DEV)
    y, dx = Guarded(1, n), Guarded(1, n)
    assert L.vc_gelu_fwd(n, P(xd), y.ptr, S()) == 0
    assert L.vc_gelu_bwd(n, P(dyd), P(xd), dx.ptr, S()) == 0
    dev_y = float((y.check()[0].double() - ref_y).abs().max())
    dev_dx = float((dx.check()[0].double() - ref_dx).abs().max())
    within("gelu_fwd", f"n={n}", dev_y, 4 * torch_dev_y + 2 * EPS32 * float(ref_y.abs().max()), inclusive=True)
    within("gelu_bwd", f"n={n}", dev_dx, 4 * torch_dev_dx + 2 * EPS32 * float(ref_dx.abs().max()), inclusive=True)
    assert L.vc_gelu_fwd(0, None, None, S()) == 0 and L.vc_gelu_bwd(0, None, None, None, S()) == 0


# ---------------------------------------------------------------------------------------------- dropout
DROP_N = 1 << 20


def dropout_fwd(L, x, add, p, seed, n=None, alias=False):
    """(y, mask) of vc_dropout_fwd over the first n elements; alias: y written over x"""
    n = x.numel() if n is None else n
    mask = Guarded(1, n, dtype=torch.uint8)
    y = Guarded(1, n, init=x[:n] if alias else None)
    xd = None if alias else x.to(DEV)
    ad = add.to(DEV) if add is not None else None
    assert L.vc_dropout_fwd(n, y.ptr if alias else P(xd), P(ad), y.ptr, mask.ptr, p, seed, S()) == 0
    return y.check()[0], mask.check()[0]


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_statistics_and_formula(L, p):
    n = DROP_N
    x, add, dy = uni(n, seed=1), uni(n, seed=2), uni(n, seed=3)
    y, mask = dropout_fwd(L, x, None, p, 1234)
    assert bool((mask <= 1).all())
    keep = mask.double()
    sd = math.sqrt(p * (1 - p) / n)
    within("dropout keep fraction", f"p={p}", abs(float(keep.mean()) - (1 - p)), 5 * sd, inclusive=True)
    # the same seed gives the same mask; another seed an independent one
    y2, mask2 = dropout_fwd(L, x, None, p, 1234)
    assert torch.equal(mask2, mask) and torch.equal(y2, y)
    _, mask3 = dropout_fwd(L, x, None, p, 987654321)
    agree_p = p * p + (1 - p) * (1 - p)
    agree = float((mask3 == mask).double().mean())
    within("dropout seed agreement", f"p={p}", abs(agree - agree_p), 5 * math.sqrt(agree_p * (1 - agree_p) / n),
           inclusive=True)
    # counter-based hash: a shorter call draws the prefix
    _, mask_short = dropout_fwd(L, x, None, p, 1234, n=1000)
    assert torch.equal(mask_short, mask[:1000])
    # y = add + keep * x / (1 - p) with the kernel's own mask
    scale32 = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    assert torch.equal(y, torch.where(mask.bool(), x * float(scale32), torch.zeros(())))
    ref = keep * x.double() / (1.0 - float(np.float32(p)))
    within("dropout_fwd", f"p={p}", rel_err(y.numpy(), ref.numpy()), 1e-6)
    ya, mask_a = dropout_fwd(L, x, add, p, 1234)
    assert torch.equal(mask_a, mask)
    within("dropout_fwd+add", f"p={p}", rel_err(ya.numpy(), (add.double() + ref).numpy()), 1e-6)
    # y aliasing x
    yi, mask_i = dropout_fwd(L, x, None, p, 1234, alias=True)
    assert torch.equal(yi, y) and torch.equal(mask_i, mask)
    yi, _ = dropout_fwd(L, x, add, p, 1234, alias=True)
    assert torch.equal(yi, ya)
    # backward: dx = mask * dy / (1 - p), out of place and over dy
    md, dyd = mask.to(DEV), dy.to(DEV)
    dx = Guarded(1, n)
    assert L.vc_dropout_bwd(n, P(dyd), P(md), p, dx.ptr, S()) == 0
    got = dx.check()[0]
    assert torch.equal(got, torch.where(mask.bool(), dy * float(scale32), torch.zeros(())))
    within("dropout_bwd", f"p={p}", rel_err(got.numpy(), (keep * dy.double() / (1.0 - float(np.float32(p)))).numpy()),
           1e-6)
    dxi = Guarded(1, n, init=dy)
    assert L.vc_dropout_bwd(n, dxi.ptr, P(md), p, dxi.ptr, S()) == 0
    assert torch.equal(dxi.check()[0], got)


def test_dropout_p0_keeps_everything(L):
    n = DROP_N
    x, dy = uni(n, seed=4), uni(n, seed=6)
    y, mask = dropout_fwd(L, x, None, 0.0, 77)
    assert bool((mask == 1).all()) and torch.equal(y, x)
    md, dyd = mask.to(DEV), dy.to(DEV)
    dx = Guarded(1, n)
    assert L.vc_dropout_bwd(n, P(dyd), P(md), 0.0, dx.ptr, S()) == 0
    assert torch.equal(dx.check()[0], dy)


# ---------------------------------------------------------------------------------------------- skip / cls kernels
BTD = [(1, 1, 1), (3, 5, 7), (2, 146, 64)]


@pytest.mark.parametrize("B,T,D", BTD)
def test_cls_rows_and_strip_cls(L, B, T, D):
    cls, pos = uni(D, seed=11), uni(T, D, seed=12)
    X = Guarded(B * T, D)
    X.view[:] = X.sent      # rows 1 .. T-1 belong to the embedding GEMM: they must stay as they are
    cd, pd = cls.to(DEV), pos.to(DEV)
    assert L.vc_s2eft_cls_rows(B, T, D, P(cd), P(pd), X.ptr, S()) == 0
    got = X.check().view(B, T, D)
    assert torch.equal(got[:, 0], (cls + pos[0]).expand(B, D))
    assert bool((got[:, 1:] == X.sent).all())
    # strip_cls over N = T tokens behind the cls row
    N = T
    dX = uni(B, N + 1, D, seed=13)
    dE = Guarded(B * N, D)
    dXd = dX.to(DEV)
    assert L.vc_s2eft_strip_cls(B, N, D, P(dXd), dE.ptr, S()) == 0
    assert torch.equal(dE.check().view(B, N, D), dX[:, 1:])


@pytest.mark.parametrize("B,T,D", BTD)
def test_skip_pack_unpack(L, B, T, D):
    x, last, bias = uni(B, T, D, seed=21), uni(B, T, D, seed=22), uni(T, seed=23)
    Z, bm = Guarded(B * T * 2, D), Guarded(T, D)
    xd, ld_, bd = x.to(DEV), last.to(DEV), bias.to(DEV)
    assert L.vc_s2eft_skip_pack(B, T, D, P(xd), P(ld_), P(bd), Z.ptr, bm.ptr, S()) == 0
    assert torch.equal(Z.check().view(B, T, 2, D), torch.stack([x, last], 2))
    assert torch.equal(bm.check(), bias[:, None].expand(T, D))
    dZ, dx0, addx = uni(B, T, 2, D, seed=24), uni(B * T, D, seed=25), uni(B * T, D, seed=26)
    dZd, ad = dZ.to(DEV), addx.to(DEV)
    for acc_x in (0, 1):
        for use_add in (False, True):
            dx = Guarded(B * T, D, init=dx0 if acc_x else None)
            dlast = Guarded(B * T, D)
            assert L.vc_s2eft_skip_unpack(B, T, D, P(dZd), dx.ptr, acc_x, P(ad) if use_add else None, dlast.ptr,
                                          S()) == 0
            got = dx.check()
            assert torch.equal(dlast.check(), dZ[:, :, 1].reshape(B * T, D))
            ref = dZ[:, :, 0].reshape(B * T, D).double()
            if not acc_x and not use_add:
                assert torch.equal(got, ref.float())
                continue
            if use_add:
                ref = ref + addx.double()
            if acc_x:
                ref = ref + dx0.double()
            within("skip_unpack", f"B={B},T={T},D={D},acc={acc_x},add={int(use_add)}",
                   rel_err(got.numpy(), ref.numpy()), 1e-6)


@pytest.mark.parametrize("B,T,D", BTD + [(5, 3, 77), (4, 2, 128)])
def test_skip_bias_grad(L, B, T, D):
    """B * D below 256 (1, 21, 128), not a multiple of 256 (385) and a multiple (512)"""
    dY = uni(B, T, D, seed=31)
    db = Guarded(1, T)
    dYd = dY.to(DEV)
    assert L.vc_s2eft_skip_bias_grad(B, T, D, P(dYd), db.ptr, S()) == 0
    within("skip_bias_grad", f"B={B},T={T},D={D}", rel_err(db.check()[0].numpy(), dY.double().sum((0, 2)).numpy()),
           1e-4)
