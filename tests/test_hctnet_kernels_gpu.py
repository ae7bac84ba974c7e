"""Per-kernel parity of csrc/hctnet.hip on the MI355X: each entry point against float64 written here from the formulas
in include/vitcnn.h (torch autograd over them gives the backward), at the smallest shapes at which it can go wrong:
1 / 4 / 6 / 8 tokens over 1 / 9 / 49 / 81 pixels, sequences of 2 / 5 / 7 / 9 rows, 1 / 3 / 5 samples, the two branches
(directions) with different weights, dropout 0 and dropout 0.1 with the kernel's own keep masks fed to the float64 side.

Outputs start as NaN and are followed by a guard region (helpers.Guarded) that must stay untouched; inputs with a
leading dimension or a branch stride sit in wider buffers whose gaps hold NaN.  Tolerance: 1e-4 of the float64 result's
max |value| per tensor (the reduction / attention class of test_s2eft_kernels_gpu.py, which test_mft_kernels_gpu.py uses
for its tokeniser and attention core).  Two runs of every backward give the same bits.  Keep fractions at p = 0.1 over
>= 2^16 mask bytes lie within test_s2eft_kernels_gpu.py's band for vc_dropout_fwd (5 standard deviations).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import Guarded, rel_err, within

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
ENC, CT = 17992, 131264   # VC_HCT_ENC_FLOATS, VC_HCT_CT_FLOATS
ENC_SHAPES = ((64,), (64,), (192, 64), (192,), (64, 64), (64,), (64,), (64,), (8, 64), (8,), (64, 8), (64,))
CT_SHAPES = ((64,), (64,), (512, 64), (1024, 64), (64, 512), (64,))


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vitcnn_amd._lib import lib
    return lib()


def S():
    return torch.cuda.current_stream().cuda_stream


def uni(*shape, seed=0, scale=0.97130763):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2.0 - 1.0) * scale


def packed(shapes, seed, norms):
    """one packed parameter block: (flat fp32 tensor, [float64 leaf per member]); `norms` are the LayerNorm weights'
    indices (drawn around 1), matrices are scaled by 1 / sqrt(fan_in)"""
    parts = []
    for i, sh in enumerate(shapes):
        t = uni(*sh, seed=seed + i)
        if i in norms:
            t = 1.0 + 0.3 * t
        elif len(sh) == 2:
            t = t / math.sqrt(sh[1])
        else:
            t = 0.3 * t
        parts.append(t)
    flat = torch.cat([p.reshape(-1) for p in parts])
    return flat, [p.double().requires_grad_(True) for p in parts]


def strided(t, stride):
    """t [2, ...] on the device with `stride` floats between the two halves, the gap NaN; returns (buffer, stride)"""
    n = t[0].numel()
    buf = torch.full((stride + n + 3,), float("nan"), device=DEV)
    buf[:n] = t[0].reshape(-1).to(DEV)
    buf[stride:stride + n] = t[1].reshape(-1).to(DEV)
    return buf


def drop64(x, mask, p):
    return x if p == 0 else x * mask.double().reshape(x.shape) / (1.0 - float(torch.tensor(p, dtype=torch.float32)))


def check_grads(name, case, got_flat, leaves):
    o = 0
    for i, w in enumerate(leaves):
        n = w.numel()
        within(f"{name} dW[{i}]", case, rel_err(got_flat[o:o + n].reshape(w.shape), w.grad), TOL)
        o += n
    assert o == got_flat.numel()


# ---------------------------------------------------------------------------------------------- tokeniser
def tok_ref(X, wA, wV, cls, pos, mask, p):
    A = torch.softmax(torch.einsum("lj,bij->bli", wA, X), dim=-1)
    U = A @ X
    T = torch.cat((cls.expand(X.shape[0], 1, 64), U @ wV), dim=1) + pos
    return A, U, drop64(T, mask, p)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("HW", [1, 9, 49, 81])
@pytest.mark.parametrize("Lt", [1, 4, 6, 8])
def test_tokpool_fwd_bwd(L, Lt, HW, B, p):
    """vc_hct_tokpool_fwd / _bwd for one source: rows with a padded leading dimension into a dense [B, L+1, 64] token
    buffer with the cls row, the position rows and the embedding dropout; dX and the reduced dwA / dwV / dpos / dcls"""
    ldx, T = 68, Lt + 1
    X = uni(B, HW, 64, seed=HW + Lt)
    wA, wV = uni(Lt, 64, seed=1) * 0.5, uni(64, 64, seed=2) * 0.2
    cls, pos, dT = uni(1, 64, seed=3), uni(T, 64, seed=4), uni(B, T, 64, seed=5)
    Xd = torch.full((B * HW, ldx), float("nan"), device=DEV)
    Xd[:, :64] = X.reshape(-1, 64).to(DEV)
    d = lambda t: t.to(DEV).contiguous()
    wAd, wVd, clsd, posd, dTd = d(wA), d(wV), d(cls), d(pos), d(dT)
    A, U, tok = Guarded(B * Lt, HW), Guarded(B * Lt, 64), Guarded(B * T, 64)
    mask = Guarded(1, B * T * 64, dtype=torch.uint8)
    L.vc_hct_tokpool_fwd(B, HW, Lt, Xd.data_ptr(), ldx, wAd.data_ptr(), wVd.data_ptr(), clsd.data_ptr(), posd.data_ptr(),
                         p, 4242, A.ptr, U.ptr, tok.ptr, mask.ptr, S())
    mk = mask.check()[0]
    assert bool((mk <= 1).all()) and (p > 0 or bool((mk == 1).all()))
    lv = [t.double().requires_grad_(True) for t in (X, wA, wV, cls, pos)]
    A64, U64, T64 = tok_ref(*lv, mk.reshape(B, T, 64), p)
    T64.backward(dT.double())
    case = (Lt, HW, B, p)
    within("vc_hct_tokpool_fwd A", case, rel_err(A.check().reshape(B, Lt, HW), A64.detach()), TOL)
    within("vc_hct_tokpool_fwd U", case, rel_err(U.check().reshape(B, Lt, 64), U64.detach()), TOL)
    within("vc_hct_tokpool_fwd T", case, rel_err(tok.check().reshape(B, T, 64), T64.detach()), TOL)
    ps = Lt * 64 + 4096 + T * 64
    ws = torch.full((B * ps,), float("nan"), device=DEV)
    outs = []
    for _ in range(2):
        dX = Guarded(B * HW, 64, ld=ldx)
        dwA, dwV, dpos, dcls = Guarded(Lt, 64), Guarded(64, 64), Guarded(T, 64), Guarded(1, 64)
        L.vc_hct_tokpool_bwd(B, HW, Lt, Xd.data_ptr(), ldx, wAd.data_ptr(), wVd.data_ptr(), A.ptr, U.ptr, dTd.data_ptr(),
                             mask.ptr, p, dX.ptr, ldx, ws.data_ptr(), B * ps, 0, dwA.ptr, dwV.ptr, dpos.ptr, dcls.ptr,
                             S())
        outs.append([g.check() for g in (dX, dwA, dwV, dpos, dcls)])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    refs = (lv[0].grad.reshape(B * HW, 64), lv[1].grad, lv[2].grad, lv[4].grad, lv[3].grad)
    for nm, got, ref in zip(("dX", "dwA", "dwV", "dpos", "dcls"), outs[0], refs):
        within(f"vc_hct_tokpool_bwd {nm}", case, rel_err(got, ref), TOL)
    # a workspace one float short is refused before any launch
    assert L.raw["vc_hct_tokpool_bwd"](B, HW, Lt, Xd.data_ptr(), ldx, wAd.data_ptr(), wVd.data_ptr(), A.ptr, U.ptr,
                                       dTd.data_ptr(), mask.ptr, p, dX.ptr, ldx, ws.data_ptr(), B * ps - 1, 0, dwA.ptr,
                                       dwV.ptr, dpos.ptr, dcls.ptr, S()) == 1


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_tokpool_two_sources_share_the_parameter_gradients(L, p):
    """the model's use: the 49-pixel source leaves its partial rows (row0 = 0, no outputs), the 81-pixel source's call
    (row0 = B) reduces both: dwA / dwV / dpos / dcls are the sums over both sources"""
    B, Lt, T = 3, 6, 7
    wA, wV = uni(Lt, 64, seed=1) * 0.5, uni(64, 64, seed=2) * 0.2
    cls, pos = uni(1, 64, seed=3), uni(T, 64, seed=4)
    d = lambda t: t.to(DEV).contiguous()
    wAd, wVd, clsd, posd = d(wA), d(wV), d(cls), d(pos)
    lv = [t.double().requires_grad_(True) for t in (wA, wV, cls, pos)]
    ps = Lt * 64 + 4096 + T * 64
    ws = torch.full((2 * B * ps,), float("nan"), device=DEV)
    dwA, dwV, dpos, dcls = Guarded(Lt, 64), Guarded(64, 64), Guarded(T, 64), Guarded(1, 64)
    keep = []
    for k, HW in enumerate((49, 81)):
        X, dT = uni(B, HW, 64, seed=10 + k), uni(B, T, 64, seed=20 + k)
        Xd, dTd = d(X.reshape(-1, 64)), d(dT)
        A, U, tok = Guarded(B * Lt, HW), Guarded(B * Lt, 64), Guarded(B * T, 64)
        mask = Guarded(1, B * T * 64, dtype=torch.uint8)
        L.vc_hct_tokpool_fwd(B, HW, Lt, Xd.data_ptr(), 64, wAd.data_ptr(), wVd.data_ptr(), clsd.data_ptr(),
                             posd.data_ptr(), p, 77 + k, A.ptr, U.ptr, tok.ptr, mask.ptr, S())
        mk = mask.check()[0]
        _, _, T64 = tok_ref(X.double(), *lv, mk.reshape(B, T, 64), p)
        T64.backward(dT.double())
        dX = Guarded(B * HW, 64)
        last = k == 1
        L.vc_hct_tokpool_bwd(B, HW, Lt, Xd.data_ptr(), 64, wAd.data_ptr(), wVd.data_ptr(), A.ptr, U.ptr, dTd.data_ptr(),
                             mask.ptr, p, dX.ptr, 64, ws.data_ptr(), 2 * B * ps, k * B, dwA.ptr if last else None,
                             dwV.ptr if last else None, dpos.ptr if last else None, dcls.ptr if last else None, S())
        keep += [Xd, dTd, A, U, tok, mask, dX]
        dX.check()
    for nm, got, ref in zip(("dwA", "dwV", "dcls", "dpos"), (dwA, dwV, dcls, dpos), lv):
        within(f"vc_hct_tokpool_bwd two sources {nm}", p, rel_err(got.check(), ref.grad.reshape(got.rows, 64)), TOL)
    # outputs given in part are refused
    assert L.raw["vc_hct_tokpool_bwd"](B, 81, Lt, Xd.data_ptr(), 64, wAd.data_ptr(), wVd.data_ptr(), A.ptr, U.ptr,
                                       dTd.data_ptr(), mask.ptr, p, dX.ptr, 64, ws.data_ptr(), 2 * B * ps, B, dwA.ptr,
                                       None, dpos.ptr, dcls.ptr, S()) == 1


# ---------------------------------------------------------------------------------------------- encoder layer
def enc_ref(x, W, m_a, m_h, m_o, p):
    ln1w, ln1b, wqkv, bqkv, wn, bn, ln2w, ln2b, w1, b1, w2, b2 = W
    B, T, _ = x.shape
    n = F.layer_norm(x, (64,), ln1w, ln1b, 1e-5)
    q, k, v = (t.reshape(B, T, 8, 8).transpose(1, 2) for t in F.linear(n, wqkv, bqkv).chunk(3, dim=-1))
    a = torch.softmax(0.125 * (q @ k.transpose(-2, -1)), dim=-1)
    o = (a @ v).transpose(1, 2).reshape(B, T, 64)
    x2 = x + drop64(F.linear(o, wn, bn), m_a, p)
    h = drop64(F.gelu(F.linear(F.layer_norm(x2, (64,), ln2w, ln2b, 1e-5), w1, b1)), m_h, p)
    return x2 + drop64(F.linear(h, w2, b2), m_o, p)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("T", [2, 5, 7, 9])
def test_encoder_fwd_bwd(L, T, B, p):
    """vc_hct_encoder_fwd / _bwd: both branches in one launch with different weights and a branch stride wider than
    the sequences; the three keep masks per branch go to the float64 side"""
    X, dY = uni(2, B, T, 64, seed=T + B), uni(2, B, T, 64, seed=T + B + 50)
    n = B * T * 64
    sx, sy, sdy, sdx = n + 20, n + 12, n + 8, n + 4
    Xd, dYd = strided(X, sx), strided(dY, sdy)
    Wf, Wl = zip(*(packed(ENC_SHAPES, 100 + 40 * br, (0, 6)) for br in (0, 1)))
    Wd = [w.to(DEV) for w in Wf]
    assert Wf[0].numel() == ENC
    Y = Guarded(1, sy + n)
    mask = Guarded(1, 2 * B * T * 136, dtype=torch.uint8)
    ps = (p,) * 6
    L.vc_hct_encoder_fwd(B, T, Xd.data_ptr(), sx, Wd[0].data_ptr(), Wd[1].data_ptr(), *ps, 991, Y.ptr, sy, mask.ptr, S())
    Yg = Y.flat[:sy + n].cpu()
    gap = Yg[n:sy].clone()
    mk = mask.check()[0].reshape(2, B, T * 136)
    assert bool((mk <= 1).all()) and (p > 0 or bool((mk == 1).all()))
    ws = torch.full((2 * B * ENC,), float("nan"), device=DEV)
    outs = []
    for _ in range(2):
        dX, dW0, dW1 = Guarded(1, sdx + n), Guarded(1, ENC), Guarded(1, ENC)
        L.vc_hct_encoder_bwd(B, T, Xd.data_ptr(), sx, Wd[0].data_ptr(), Wd[1].data_ptr(), *ps, mask.ptr, dYd.data_ptr(),
                             sdy, dX.ptr, sdx, dW0.ptr, dW1.ptr, ws.data_ptr(), 2 * B * ENC, S())
        outs.append([dW0.check()[0], dW1.check()[0], dX.flat[:sdx + n].cpu()])
    assert all(torch.equal(a[~a.isnan()], b[~b.isnan()]) for a, b in zip(*outs))
    Y.check()
    assert bool(gap.isnan().all()) and bool(outs[0][2][n:sdx].isnan().all())   # nothing between the branches
    case = (T, B, p)
    for br in (0, 1):
        x64 = X[br].double().requires_grad_(True)
        m = mk[br]
        y64 = enc_ref(x64, Wl[br], m[:, :T * 64].reshape(B, T, 64), m[:, T * 64:T * 72].reshape(B, T, 8),
                      m[:, T * 72:].reshape(B, T, 64), p)
        y64.backward(dY[br].double())
        o = br * sy
        within(f"vc_hct_encoder_fwd Y[{br}]", case, rel_err(Yg[o:o + n].reshape(B, T, 64), y64.detach()), TOL)
        o = br * sdx
        within(f"vc_hct_encoder_bwd dX[{br}]", case, rel_err(outs[0][2][o:o + n].reshape(B, T, 64), x64.grad), TOL)
        check_grads(f"vc_hct_encoder_bwd[{br}]", case, outs[0][br], Wl[br])
    assert L.raw["vc_hct_encoder_bwd"](B, T, Xd.data_ptr(), sx, Wd[0].data_ptr(), Wd[1].data_ptr(), *ps, mask.ptr,
                                       dYd.data_ptr(), sdy, dX.ptr, sdx, dW0.ptr, dW1.ptr, ws.data_ptr(),
                                       2 * B * ENC - 1, S()) == 1


def test_encoder_rejects_bad_shapes(L):
    x = torch.zeros(2 * 10 * 64, device=DEV)
    w = torch.zeros(ENC, device=DEV)
    args = lambda T, st, p: (1, T, x.data_ptr(), st, w.data_ptr(), w.data_ptr(), p, 0.0, 0.0, 0.0, 0.0, 0.0, 0, x.data_ptr(),
                             st, None, S())
    raw = L.raw["vc_hct_encoder_fwd"]
    assert raw(*args(1, 640, 0.0)) == 1 and raw(*args(10, 640, 0.0)) == 1      # T outside 2..9
    assert raw(*args(5, 319, 0.0)) == 1                                          # branches overlap
    assert raw(*args(5, 320, 0.1)) == 1 and raw(*args(5, 320, 1.0)) == 1         # dropout without a mask; p = 1


# ---------------------------------------------------------------------------------------------- cross-token step
def ct_ref(x, other, W, m_p, m_o, p):
    lnw, lnb, wq, wkv, wo, bo = W
    B, T, _ = x.shape
    cls = x[:, :1]
    c0 = F.layer_norm(cls, (64,), lnw, lnb, 1e-5)
    ctx = torch.cat((c0, other[:, 1:]), dim=1)
    q = F.linear(c0, wq).reshape(B, 1, 8, 64).transpose(1, 2)
    k, v = (t.reshape(B, T, 8, 64).transpose(1, 2) for t in F.linear(ctx, wkv).chunk(2, dim=-1))
    a = drop64(torch.softmax(0.125 * (q @ k.transpose(-2, -1)), dim=-1), m_p, p)
    o = (a @ v).transpose(1, 2).reshape(B, 1, 512)
    return (cls + drop64(F.linear(o, wo, bo), m_o, p))[:, 0]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("T", [2, 5, 7, 9])
def test_ctattn_fwd_bwd(L, T, B, p):
    """vc_hct_ctattn_fwd / _bwd: both directions in one launch with different weights; direction d writes the gradient
    of branch d's row 0 and of branch 1 - d's rows 1..; the keep masks go to the float64 side"""
    X, dO = uni(2, B, T, 64, seed=T + B + 7), uni(2, B, 64, seed=T + B + 70)
    n = B * T * 64
    sx, sdx = n + 20, n + 4
    Xd, dOd = strided(X, sx), dO.to(DEV).contiguous()
    Wf, Wl = zip(*(packed(CT_SHAPES, 300 + 40 * d, (0,)) for d in (0, 1)))
    Wd = [w.to(DEV) for w in Wf]
    assert Wf[0].numel() == CT
    out = Guarded(2 * B, 64)
    mask = Guarded(1, 2 * B * (8 * T + 64), dtype=torch.uint8)
    ps = (p,) * 4
    L.vc_hct_ctattn_fwd(B, T, Xd.data_ptr(), sx, Wd[0].data_ptr(), Wd[1].data_ptr(), *ps, 55, out.ptr, mask.ptr, S())
    og = out.check().reshape(2, B, 64)
    mk = mask.check()[0].reshape(2, B, 8 * T + 64)
    assert bool((mk <= 1).all()) and (p > 0 or bool((mk == 1).all()))
    ws = torch.full((2 * B * CT,), float("nan"), device=DEV)
    outs = []
    for _ in range(2):
        dX, dW0, dW1 = Guarded(1, sdx + n), Guarded(1, CT), Guarded(1, CT)
        L.vc_hct_ctattn_bwd(B, T, Xd.data_ptr(), sx, Wd[0].data_ptr(), Wd[1].data_ptr(), *ps, mask.ptr, dOd.data_ptr(),
                            dX.ptr, sdx, dW0.ptr, dW1.ptr, ws.data_ptr(), 2 * B * CT, S())
        outs.append([dW0.check()[0], dW1.check()[0], dX.flat[:sdx + n].cpu()])
    assert all(torch.equal(a[~a.isnan()], b[~b.isnan()]) for a, b in zip(*outs))
    assert bool(outs[0][2][n:sdx].isnan().all())
    case = (T, B, p)
    x64 = X.double().requires_grad_(True)
    for d in (0, 1):
        m = mk[d]
        y64 = ct_ref(x64[d], x64[1 - d], Wl[d], m[:, :8 * T].reshape(B, 8, 1, T), m[:, 8 * T:].reshape(B, 1, 64), p)
        y64.backward(dO[d].double())
        within(f"vc_hct_ctattn_fwd out[{d}]", case, rel_err(og[d], y64.detach()), TOL)
        check_grads(f"vc_hct_ctattn_bwd[{d}]", case, outs[0][d], Wl[d])
    got = torch.stack([outs[0][2][:n], outs[0][2][sdx:sdx + n]]).reshape(2, B, T, 64)
    assert not got.isnan().any()      # every element of both branches written by exactly one direction
    within("vc_hct_ctattn_bwd dX", case, rel_err(got, x64.grad), TOL)
    assert L.raw["vc_hct_ctattn_bwd"](B, T, Xd.data_ptr(), sx, Wd[0].data_ptr(), Wd[1].data_ptr(), *ps, mask.ptr,
                                      dOd.data_ptr(), dX.ptr, sdx, dW0.ptr, dW1.ptr, ws.data_ptr(), 2 * B * CT - 1,
                                      S()) == 1


# ---------------------------------------------------------------------------------------------- keep fractions
def _band(mk, p):
    n = mk.numel()
    assert n >= 1 << 16
    within("keep fraction", n, abs(float(mk.double().mean()) - (1 - p)), 5 * math.sqrt(p * (1 - p) / n), inclusive=True)


def test_keep_fractions(L):
    """p = 0.1 over >= 2^16 mask bytes per kernel: within 5 standard deviations of 0.9 (vc_dropout_fwd's band); the same
    seed gives the same mask, another seed another"""
    p = 0.1
    z = lambda *s: torch.zeros(*s, device=DEV)
    # tokeniser: B 128, 8 tokens, 9 pixels -> 73728 bytes
    B, Lt, HW = 128, 8, 9
    X, wA, wV, cls, pos = uni(B * HW, 64).to(DEV), z(Lt, 64), z(64, 64), z(64), z(Lt + 1, 64)
    A, U, T = z(B, Lt, HW), z(B, Lt, 64), z(B, Lt + 1, 64)
    mks = []
    for seed in (1, 1, 2):
        mask = Guarded(1, B * (Lt + 1) * 64, dtype=torch.uint8)
        L.vc_hct_tokpool_fwd(B, HW, Lt, X.data_ptr(), 64, wA.data_ptr(), wV.data_ptr(), cls.data_ptr(), pos.data_ptr(), p,
                             seed, A.data_ptr(), U.data_ptr(), T.data_ptr(), mask.ptr, S())
        mks.append(mask.check()[0])
    _band(mks[0], p)
    assert torch.equal(mks[0], mks[1]) and not torch.equal(mks[0], mks[2])
    # encoder: B 32, T 9 -> 78336 bytes
    B, T = 32, 9
    Xe, W = uni(2, B, T, 64).to(DEV), packed(ENC_SHAPES, 5, (0, 6))[0].to(DEV)
    Y = z(2, B, T, 64)
    mask = Guarded(1, 2 * B * T * 136, dtype=torch.uint8)
    L.vc_hct_encoder_fwd(B, T, Xe.data_ptr(), B * T * 64, W.data_ptr(), W.data_ptr(), p, p, p, p, p, p, 3, Y.data_ptr(),
                         B * T * 64, mask.ptr, S())
    _band(mask.check()[0], p)
    # cross-token step: B 256, T 9 -> 69632 bytes
    B = 256
    Xc, Wc = uni(2, B, T, 64).to(DEV), packed(CT_SHAPES, 9, (0,))[0].to(DEV)
    out = z(2, B, 64)
    mask = Guarded(1, 2 * B * (8 * T + 64), dtype=torch.uint8)
    L.vc_hct_ctattn_fwd(B, T, Xc.data_ptr(), B * T * 64, Wc.data_ptr(), Wc.data_ptr(), p, p, p, p, 4, out.data_ptr(),
                        mask.ptr, S())
    _band(mask.check()[0], p)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(Y).all())
