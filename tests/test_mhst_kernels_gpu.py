"""Every MHST kernel (csrc/mhst.hip) against float64 written from the formulas in include/vitcnn.h, with guarded outputs
and poisoned inputs, at the smallest shapes at which each can still go wrong.  Bound: 1e-4 of the tensor's largest
magnitude, the kernel classes' bound (DESIGN.md sections 16 and 22)."""
import math

import pytest
import torch
import torch.nn.functional as F

import mhst_oracle as O
from helpers import GUARD, SENTINEL, Guarded, Poisoned, within

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
    want = want.reshape(got.shape)
    within(kernel, shape, float((got.double() - want).abs().max()), BOUND * max(float(want.abs().max()), 1e-30))


# (B, D, C, O, G, KD, KS, sd, pd, ldx, ycol, ldy): the model's seven kinds of convolution
CONVS = {
    "conv1 l1=1": (2, 1, 1, 16, 1, 11, 3, 3, 5, 1, 0, 16),
    "conv1 l1=2": (2, 2, 1, 16, 1, 11, 3, 3, 5, 1, 0, 16),
    "conv1 l1=4": (3, 4, 1, 16, 1, 11, 3, 3, 5, 1, 0, 16),
    "conv1 l1=11": (2, 11, 1, 16, 1, 11, 3, 3, 5, 1, 0, 16),
    "conv1 l1=30": (1, 30, 1, 16, 1, 11, 3, 3, 5, 1, 0, 16),
    "spectral 1 tap": (2, 4, 16, 4, 1, 1, 1, 1, 0, 16, 0, 16),
    "spectral 5 taps into columns 8..11": (2, 2, 16, 4, 1, 5, 1, 1, 2, 16, 8, 16),
    "spectral 11 taps at depth 4": (1, 4, 16, 4, 1, 11, 1, 1, 5, 16, 12, 16),
    "3x3x3 depth 1": (2, 1, 16, 16, 1, 3, 3, 1, 1, 16, 0, 16),
    "3x3x3 depth 10": (1, 10, 16, 16, 1, 3, 3, 1, 1, 16, 0, 16),
    "pyconv 16 ch k3 g1": (2, 1, 16, 16, 1, 1, 3, 1, 0, 16, 0, 64),
    "pyconv 16 ch k5 g2": (2, 1, 16, 16, 2, 1, 5, 1, 0, 16, 16, 64),
    "pyconv 16 ch k7 g4": (2, 1, 16, 16, 4, 1, 7, 1, 0, 16, 32, 64),
    "pyconv 16 ch k9 g8 (2 per group)": (2, 1, 16, 16, 8, 1, 9, 1, 0, 16, 48, 64),
    "pyconv 48 ch k3 g1": (2, 3, 16, 16, 1, 3, 3, 1, 0, 16, 0, 64),
    "pyconv 48 ch k5 g2": (2, 3, 16, 16, 2, 3, 5, 1, 0, 16, 16, 64),
    "pyconv 48 ch k7 g4": (1, 3, 16, 16, 4, 3, 7, 1, 0, 16, 32, 64),
    "pyconv 48 ch k9 g8 (6 per group)": (3, 3, 16, 16, 8, 3, 9, 1, 0, 16, 48, 64),
    "lidar 1 band k9": (2, 1, 1, 8, 1, 1, 9, 1, 0, 4, 24, 32),
    "lidar 2 bands k5": (3, 1, 2, 8, 1, 1, 5, 1, 0, 4, 8, 32),
    "lidar 3 bands k7": (2, 1, 3, 8, 1, 1, 7, 1, 0, 4, 16, 32),
    "lidar 1 band k3, rows of 1 float": (2, 1, 1, 8, 1, 1, 3, 1, 0, 1, 0, 32),
    "lidar 3 bands k9, rows of 3 floats": (2, 1, 3, 8, 1, 1, 9, 1, 0, 3, 24, 32),
    "lidar 32 -> 16 k3": (2, 1, 32, 16, 1, 1, 3, 1, 0, 32, 0, 64),
    "classifier k5 g2": (2, 1, 64, 16, 2, 1, 5, 1, 0, 64, 16, 32),
}


@pytest.mark.parametrize("name", list(CONVS))
def test_conv_family(name):
    B, D, C, O, G, KD, KS, sd, pd, ldx, ycol, ldy = CONVS[name]
    Dout = (D + 2 * pd - KD) // sd + 1
    shape = (D, 8, 8, C, O, G, KD, KS, sd, pd, Dout)
    g = torch.Generator().manual_seed(1)
    x = rnd(g, B, C, D, 8, 8).requires_grad_(True)
    w = rnd(g, O, C // G, KD, KS, KS).requires_grad_(True)
    bias = rnd(g, O).requires_grad_(True)
    dy = rnd(g, B, O, Dout, 8, 8)
    y = F.conv3d(x, w, bias, stride=(sd, 1, 1), padding=(pd, KS // 2, KS // 2), groups=G)
    y.backward(dy)
    rows = lambda t: t.detach().permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])   # noqa: E731  channels-last rows
    xd = Poisoned(rows(x).float(), ld=ldx)
    wd = Poisoned(w.detach().reshape(1, -1).float(), lead=1)
    bd = Poisoned(bias.detach().reshape(1, -1).float(), lead=3)
    Mo = B * Dout * 64
    # the part's O columns start at column ycol of rows of ldy: everything else in the buffer must stay untouched
    flat = torch.full((Mo * ldy + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    L().vc_mhst_conv_fwd(B, *shape, xd.ptr, ldx, wd.ptr, bd.ptr, flat.data_ptr() + 4 * ycol, ldy, stream())
    torch.cuda.synchronize()
    flat = flat.cpu()
    close("vc_mhst_conv_fwd", name, flat.as_strided((Mo, O), (ldy, 1), ycol).clone(), rows(y))
    flat.as_strided((Mo, O), (ldy, 1), ycol).fill_(SENTINEL)
    assert bool((flat == SENTINEL).all()), "store outside the part's columns"
    dyd = Poisoned(rows(dy).float(), ld=O + 3)
    init = rnd(g, B * D * 64, C).float()
    for beta in (0.0, 1.0):
        dxg = Guarded(B * D * 64, C, ld=ldx, init=init if beta else None)
        L().vc_mhst_conv_dgrad(B, *shape, dyd.ptr, O + 3, wd.ptr, dxg.ptr, ldx, beta, stream())
        close("vc_mhst_conv_dgrad", f"{name} beta {beta}", dxg.check(), rows(x.grad) + beta * init.double())
    dwg, dbg = Guarded(1, w.numel()), Guarded(1, O)
    L().vc_mhst_conv_wgrad(B, *shape, xd.ptr, ldx, dyd.ptr, O + 3, dwg.ptr, dbg.ptr, stream())
    close("vc_mhst_conv_wgrad", name, dwg.check(), w.grad)
    close("vc_mhst_conv_wgrad bias", name, dbg.check(), bias.grad)
    dwg = Guarded(1, w.numel())
    L().vc_mhst_conv_wgrad(B, *shape, xd.ptr, ldx, dyd.ptr, O + 3, dwg.ptr, None, stream())
    close("vc_mhst_conv_wgrad no bias", name, dwg.check(), w.grad)


@pytest.mark.parametrize("B,D,ld", [(2, 1, 16), (3, 2, 20), (1, 10, 16), (5, 3, 16), (130, 4, 16)])
def test_conv3_mfma(B, D, ld):
    """the 3x3x3 conv on the MFMA: depth 1 (both neighbour planes in the padding), 2, more planes than one wave of the
    weight gradient's grid takes in one pass (B D = 520 > 512), rows of 20 floats"""
    g = torch.Generator().manual_seed(8)
    x = rnd(g, B, 16, D, 8, 8).requires_grad_(True)
    w = rnd(g, 16, 16, 3, 3, 3).requires_grad_(True)
    bias = rnd(g, 16).requires_grad_(True)
    dy = rnd(g, B, 16, D, 8, 8)
    y = F.conv3d(x, w, bias, padding=1)
    y.backward(dy)
    rows = lambda t: t.detach().permute(0, 2, 3, 4, 1).reshape(-1, 16)   # noqa: E731
    M = B * D * 64
    xd, dyd = Poisoned(rows(x).float(), ld=ld), Poisoned(rows(dy).float(), ld=ld)
    wd, bd = Poisoned(w.detach().reshape(1, -1).float(), lead=1), Poisoned(bias.detach().reshape(1, -1).float(), lead=3)
    yg = Guarded(M, 16, ld=ld + 3)
    L().vc_mhst_conv3_fwd(B, D, xd.ptr, ld, wd.ptr, bd.ptr, yg.ptr, ld + 3, stream())
    close("vc_mhst_conv3_fwd", (B, D, ld), yg.check(), rows(y))
    yg = Guarded(M, 16)
    L().vc_mhst_conv3_fwd(B, D, xd.ptr, ld, wd.ptr, None, yg.ptr, 16, stream())
    close("vc_mhst_conv3_fwd no bias", (B, D, ld), yg.check(), rows(y) - bias.detach())
    init = rnd(g, M, 16).float()
    for beta in (0.0, 1.0):
        dxg = Guarded(M, 16, ld=17, init=init if beta else None)
        L().vc_mhst_conv3_dgrad(B, D, dyd.ptr, ld, wd.ptr, dxg.ptr, 17, beta, stream())
        close("vc_mhst_conv3_dgrad", (B, D, ld, beta), dxg.check(), rows(x.grad) + beta * init.double())
    n = L().vc_mhst_conv3_wgrad_ws_floats(B, D)
    assert n == min(512, B * D) * 6912
    ws, dwg = Guarded(1, n), Guarded(1, 6912)
    L().vc_mhst_conv3_wgrad(B, D, xd.ptr, ld, dyd.ptr, ld, dwg.ptr, ws.ptr, n, stream())
    got = dwg.check()
    ws.check()
    close("vc_mhst_conv3_wgrad", (B, D, ld), got, w.grad)
    dwg2 = Guarded(1, 6912)
    L().vc_mhst_conv3_wgrad(B, D, xd.ptr, ld, dyd.ptr, ld, dwg2.ptr, ws.ptr, n, stream())
    assert torch.equal(dwg2.check(), got)      # a second run: the same bits


@pytest.mark.parametrize("B", [1, 3])
def test_embed(B):
    g = torch.Generator().manual_seed(2)
    ph, pl = rnd(g, B, 16, 64).requires_grad_(True), rnd(g, B, 16, 64).requires_grad_(True)
    wh, wl = rnd(g, 1).requires_grad_(True), rnd(g, 1).requires_grad_(True)
    W, bias = rnd(g, 64, 16).requires_grad_(True), rnd(g, 64).requires_grad_(True)
    pos, cls = rnd(g, 65, 64).requires_grad_(True), rnd(g, 64).requires_grad_(True)
    f = wh * ph + wl * pl
    xcnn = torch.einsum("jp,bpc->bjc", W, f) + bias[None, :, None]
    X0 = torch.cat([cls.expand(B, 1, 64), xcnn + pos[1:]], dim=1) + pos[:1]
    dX0, dxc = rnd(g, B, 65, 64), rnd(g, B, 64, 64)
    (X0 * dX0).sum().backward(retain_graph=True)
    (xcnn * dxc).sum().backward()
    P2 = lambda t, **kw: Poisoned(t.detach().reshape(-1, t.shape[-1]).float(), **kw)   # noqa: E731
    d = dict(ph=P2(ph), pl=P2(pl), wh=P2(wh.reshape(1, 1), lead=1), wl=P2(wl.reshape(1, 1), lead=2), W=P2(W),
             bias=P2(bias.reshape(1, -1)), pos=P2(pos), cls=P2(cls.reshape(1, -1)), dX0=P2(dX0), dxc=P2(dxc))
    xg, Xg = Guarded(B * 64, 64), Guarded(B * 65, 64)
    L().vc_mhst_embed_fwd(B, d["ph"].ptr, d["pl"].ptr, d["wh"].ptr, d["wl"].ptr, d["W"].ptr, d["bias"].ptr, d["pos"].ptr,
                          d["cls"].ptr, xg.ptr, Xg.ptr, stream())
    close("vc_mhst_embed_fwd xcnn", B, xg.check(), xcnn.detach())
    close("vc_mhst_embed_fwd X0", B, Xg.check(), X0.detach())
    dphg, dplg, part = Guarded(B * 16, 64), Guarded(B * 16, 64), Guarded(B, 1156)
    L().vc_mhst_embed_bwd(B, d["ph"].ptr, d["pl"].ptr, d["wh"].ptr, d["wl"].ptr, d["W"].ptr, d["dX0"].ptr, d["dxc"].ptr,
                          dphg.ptr, dplg.ptr, part.ptr, stream())
    close("vc_mhst_embed_bwd dph", B, dphg.check(), ph.grad)
    close("vc_mhst_embed_bwd dpl", B, dplg.check(), pl.grad)
    p = part.check().double().sum(0)
    close("vc_mhst_embed_bwd dW", B, p[:1024], W.grad)
    close("vc_mhst_embed_bwd dbias", B, p[1024:1088], bias.grad)
    close("vc_mhst_embed_bwd dpos0", B, p[1088:1152], pos.grad[0])
    close("vc_mhst_embed_bwd dwh dwl", B, p[1152:1154], torch.cat([wh.grad, wl.grad]))
    assert not p[1154:].any()


@pytest.mark.parametrize("train", [0, 1])
def test_gate_with_supplied_noise(train):
    B, T = 3, 65
    g = torch.Generator().manual_seed(3)
    X, Wg, bg, nz = rnd(g, B, T * 64), rnd(g, 16, 64), rnd(g, 16), 3 * rnd(g, B, 16)
    logits = X[:, :64] @ Wg.T + bg
    v = (logits + nz) / 5.0 if train else logits
    Xd, Wd, bd, nd = Poisoned(X.float()), Poisoned(Wg.float()), Poisoned(bg.reshape(1, -1).float(), lead=1), \
        Poisoned(nz.float())
    lg, no, yg, sg = (Guarded(B, 16) for _ in range(4))
    L().vc_mhst_gate_fwd(B, Xd.ptr, T * 64, Wd.ptr, bd.ptr, nd.ptr, train, 5.0, 0, lg.ptr, no.ptr, yg.ptr, sg.ptr, stream())
    close("vc_mhst_gate_fwd logits", train, lg.check(), logits)
    close("vc_mhst_gate_fwd y", train, yg.check(), torch.sigmoid(v))
    sel = sg.check().double()
    far = v.abs() > 1e-4
    assert torch.equal(sel[far], (v > 0).double()[far])
    assert torch.equal(no.check().double(), nz.float().double() if train else torch.zeros(B, 16, dtype=torch.float64))
    dsel = rnd(g, B, 16)
    dl = Guarded(B, 16)
    scale = 0.2 if train else 1.0
    dsd = Poisoned(dsel.float())
    L().vc_mhst_gate_bwd(B, dsd.ptr, yg.ptr, scale, dl.ptr, stream())
    y = torch.sigmoid(v)
    close("vc_mhst_gate_bwd", train, dl.check(), dsel * y * (1 - y) * scale)


def test_gate_noise_is_logistic_and_ds_twin_matches():
    """Logistic(0, 1): mean 0, variance pi^2 / 3; 5-sigma bands over 64k draws (the variance of the squared deviate is
    the fourth central moment 7 pi^4 / 15 minus the variance squared)"""
    B = 4096
    X, Wg, bg = torch.zeros(B, 64, device="cuda"), torch.zeros(16, 64, device="cuda"), torch.zeros(16, device="cuda")
    outs = []
    seed = 123456789
    sd = torch.tensor([seed - 77], dtype=torch.int64, device="cuda")
    for ds in (False, True):
        lg, no, yg, sg = (Guarded(B, 16) for _ in range(4))
        if ds:
            L().vc_mhst_gate_fwd_ds(B, X.data_ptr(), 64, Wg.data_ptr(), bg.data_ptr(), None, 1, 5.0, sd.data_ptr(), 77,
                                    lg.ptr, no.ptr, yg.ptr, sg.ptr, stream())
        else:
            L().vc_mhst_gate_fwd(B, X.data_ptr(), 64, Wg.data_ptr(), bg.data_ptr(), None, 1, 5.0, seed, lg.ptr, no.ptr,
                                 yg.ptr, sg.ptr, stream())
        outs.append((no.check(), sg.check()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    nz = outs[0][0].double().reshape(-1)
    n = nz.numel()
    assert n >= 65536 and bool(torch.isfinite(nz).all())
    var = math.pi ** 2 / 3
    within("gate noise mean", n, abs(float(nz.mean())), 5 * math.sqrt(var / n))
    m4 = 7 * math.pi ** 4 / 15
    within("gate noise variance", n, abs(float((nz ** 2).mean()) - var), 5 * math.sqrt((m4 - var ** 2) / n))
    assert torch.equal(outs[0][1].double().reshape(-1), (nz > 0).double())


@pytest.mark.parametrize("Wd", [64, 192])
@pytest.mark.parametrize("heads", ["none", "all", "one", "mixed"])
def test_headmask(Wd, heads):
    B = 1 if heads != "mixed" else 3
    g = torch.Generator().manual_seed(4)
    sel = {"none": torch.zeros(B, 16), "all": torch.ones(B, 16), "one": F.one_hot(torch.tensor([5]), 16).float(),
           "mixed": (torch.rand(B, 16, generator=g) > 0.5).float()}[heads].double()
    X, dY, d0 = rnd(g, B, 65, Wd), rnd(g, B, 65, Wd), rnd(g, B, 16)
    wide = sel.repeat_interleave(4, dim=1).repeat(1, Wd // 64)[:, None, :]
    Xd, dYd, sd = Poisoned(X.reshape(-1, Wd).float()), Poisoned(dY.reshape(-1, Wd).float()), Poisoned(sel.float())
    Yg = Guarded(B * 65, Wd)
    L().vc_mhst_headmask_fwd(B, 65, Wd, Xd.ptr, sd.ptr, Yg.ptr, stream())
    assert torch.equal(Yg.check().double(), (X.float().double() * wide).reshape(-1, Wd))
    want = (dY * X).reshape(B, 65, Wd // 64, 16, 4).sum((1, 2, 4))
    for beta in (0.0, 1.0):
        dXg, dsg = Guarded(B * 65, Wd), Guarded(B, 16, init=d0.float() if beta else None)
        L().vc_mhst_headmask_bwd(B, 65, Wd, dYd.ptr, Xd.ptr, sd.ptr, dXg.ptr, dsg.ptr, beta, stream())
        assert torch.equal(dXg.check().double(), (dY.float().double() * wide).reshape(-1, Wd))
        close("vc_mhst_headmask_bwd dsel", (Wd, heads, beta), dsg.check(), want + beta * d0.float().double())


def _pool_params(g):
    P, flat = {}, []
    for n in "qkv":
        P[f"a.pool_{n}.weight"] = rnd(g, 4, 1, 3, 3).requires_grad_(True)
        P[f"a.norm_{n}.weight"] = (1 + 0.5 * rnd(g, 4)).requires_grad_(True)
        P[f"a.norm_{n}.bias"] = rnd(g, 4).requires_grad_(True)
        flat += [P[f"a.pool_{n}.weight"], P[f"a.norm_{n}.weight"], P[f"a.norm_{n}.bias"]]
    return P, flat


@pytest.mark.parametrize("heads", ["none", "all", "one", "mixed"])
def test_pool(heads):
    """a switched-off head's rows are exactly zero going in and come out as the norm's bias (rstd = eps^-0.5)"""
    B = 1 if heads != "mixed" else 2
    g = torch.Generator().manual_seed(5)
    sel = {"none": torch.zeros(B, 16), "all": torch.ones(B, 16), "one": F.one_hot(torch.tensor([9]), 16).float(),
           "mixed": (torch.rand(B, 16, generator=g) > 0.5).float()}[heads].double()
    P, flat = _pool_params(g)
    X = (rnd(g, B, 65, 192) * sel.repeat_interleave(4, dim=1).repeat(1, 3)[:, None, :]).requires_grad_(True)
    dY = rnd(g, B, 65, 192)
    Y = torch.cat([O.attn_pool(P, "a.", n, X[:, :, 64 * i:64 * i + 64]).transpose(1, 2).reshape(B, 65, 64)
                   for i, n in enumerate("qkv")], dim=2)
    Y.backward(dY)
    pw = Poisoned(torch.cat([t.detach().reshape(-1) for t in flat]).reshape(1, -1).float(), lead=1)
    Xd, dYd = Poisoned(X.detach().reshape(-1, 192).float()), Poisoned(dY.reshape(-1, 192).float())
    Yg = Guarded(B * 65, 192)
    L().vc_mhst_pool_fwd(B, Xd.ptr, pw.ptr, 1e-5, Yg.ptr, stream())
    got = Yg.check()
    close("vc_mhst_pool_fwd", heads, got, Y.detach())
    off = (sel == 0).repeat_interleave(4, dim=1).repeat(1, 3)[:, None, :].expand(B, 65, 192)
    bias = torch.cat([P[f"a.norm_{n}.bias"].detach().float().repeat(16) for n in "qkv"]).expand(B, 65, 192)
    assert torch.equal(got.reshape(B, 65, 192)[off], bias[off])
    dXg, part = Guarded(B * 65, 192), Guarded(B, 132)
    L().vc_mhst_pool_bwd(B, Xd.ptr, pw.ptr, 1e-5, dYd.ptr, dXg.ptr, part.ptr, stream())
    close("vc_mhst_pool_bwd dX", heads, dXg.check(), X.grad)
    close("vc_mhst_pool_bwd params", heads, part.check().double().sum(0), torch.cat([t.grad.reshape(-1) for t in flat]))


@pytest.mark.parametrize("heads,p,train", [("none", 0.0, 1), ("all", 0.1, 1), ("one", 0.0, 1), ("mixed", 0.1, 1),
                                           ("mixed", 0.0, 0)])
def test_hsattn_fused(heads, p, train):
    """the fused chain gate -> head mask -> pooling -> attention -> head mask against float64 (the gate's decisions
    adopted; they are checked against v > 0 away from ties), forward and backward, with all heads off, all on, one on
    (B = 1) and mixed (B = 3); the straight-through gradient reaches the logits from all three masks"""
    B = 3 if heads == "mixed" else 1
    g = torch.Generator().manual_seed(9)
    X, Wg, nz = rnd(g, B, 65 * 64), rnd(g, 16, 64), 3 * rnd(g, B, 16)
    # a bias of +-25 decides every head and leaves y (1 - y) well inside fp32 (|v| about 5: 1 - y is not a cancellation)
    bg = {"none": torch.full((16,), -25.0), "all": torch.full((16,), 25.0),
          "one": torch.where(torch.arange(16) == 11, 25.0, -25.0), "mixed": rnd(g, 16).float()}[heads].double()
    P, flat = _pool_params(g)
    QKV = (2 * rnd(g, B, 65, 192)).requires_grad_(True)
    dAM, dsel_in = rnd(g, B, 65, 64), rnd(g, B, 16)
    Xd, Wd, bd, nd = Poisoned(X.float()), Poisoned(Wg.float()), Poisoned(bg.reshape(1, -1).float(), lead=1), \
        Poisoned(nz.float())
    Qd = Poisoned(QKV.detach().reshape(-1, 192).float())
    pw = Poisoned(torch.cat([t.detach().reshape(-1) for t in flat]).reshape(1, -1).float(), lead=1)
    lg, no, yg, sg = (Guarded(B, 16) for _ in range(4))
    mk, AM = Guarded(B * 16 * 65, 65, dtype=torch.uint8), Guarded(B * 65, 64)
    L().vc_mhst_hsattn_fwd(B, Xd.ptr, 65 * 64, Wd.ptr, bd.ptr, nd.ptr, train, 5.0, 0, 777, Qd.ptr, pw.ptr, 1e-5, 0.5, p,
                           mk.ptr, lg.ptr, no.ptr, yg.ptr, sg.ptr, AM.ptr, stream())
    sel = sg.check().double()
    keep = mk.check().double().reshape(B, 16, 65, 65)
    logits = (X[:, :64] @ Wg.T + bg).requires_grad_(True)
    v = (logits + nz.float().double()) / 5.0 if train else logits
    yv = torch.sigmoid(v)
    far = v.detach().abs() > 1e-4
    assert torch.equal(sel[far], (v.detach() > 0).double()[far])
    assert {"none": sel.sum() == 0, "all": sel.sum() == 16, "one": sel.sum() == 1, "mixed": 0 < sel.sum() < 16 * B}[heads]
    st = sel - yv.detach() + yv
    w4 = st.repeat_interleave(4, dim=1)[:, None, :]
    qm = QKV * w4.repeat(1, 1, 3)
    q, k, vv = (O.attn_pool(P, "a.", n, qm[:, :, 64 * i:64 * i + 64]) for i, n in enumerate("qkv"))
    at = torch.softmax(q @ k.transpose(-1, -2) * 0.5, dim=-1) * keep / (1 - p)
    ao = at @ vv + torch.cat([torch.zeros_like(q[:, :, :1]), q[:, :, 1:]], dim=2)
    am = ao.transpose(1, 2).reshape(B, 65, 64) * w4
    ((am * dAM).sum() + (st * dsel_in).sum()).backward()
    close("vc_mhst_hsattn_fwd logits", (heads, p, train), lg.check(), logits.detach())
    close("vc_mhst_hsattn_fwd y", (heads, p, train), yg.check(), yv.detach())
    close("vc_mhst_hsattn_fwd AM", (heads, p, train), AM.check(), am.detach())
    assert torch.equal(no.check().double(), nz.float().double() if train else torch.zeros(B, 16, dtype=torch.float64))
    if heads == "none":
        assert not AM.check().any()
    if p > 0:   # the same keep bytes as the unfused attention's at the same seed
        mk2, O2 = Guarded(B * 16 * 65, 65, dtype=torch.uint8), Guarded(B * 65, 64)
        L().vc_mhst_attn_fwd(B, Qd.ptr, 0.5, p, 777, mk2.ptr, O2.ptr, stream())
        assert torch.equal(mk2.check(), mk.check())
    dAMd, dsd = Poisoned(dAM.reshape(-1, 64).float()), Poisoned(dsel_in.float())
    dQ, part, dl = Guarded(B * 65, 192), Guarded(B * 16, 132), Guarded(B, 16)
    scale = 0.2 if train else 1.0
    L().vc_mhst_hsattn_bwd(B, Qd.ptr, sg.ptr, yg.ptr, pw.ptr, 1e-5, 0.5, p, mk.ptr if p > 0 else None, dAMd.ptr, dsd.ptr,
                           scale, dQ.ptr, part.ptr, dl.ptr, stream())
    close("vc_mhst_hsattn_bwd dQKV", (heads, p, train), dQ.check(), QKV.grad)
    close("vc_mhst_hsattn_bwd params", (heads, p, train), part.check().double().sum(0),
          torch.cat([t.grad.reshape(-1) for t in flat]))
    want = logits.grad * (5.0 if train else 1.0) * scale     # autograd's 1 / tau is the kernel's gscale
    close("vc_mhst_hsattn_bwd dlogits", (heads, p, train), dl.check(), want)
    dl2 = Guarded(B, 16)
    L().vc_mhst_hsattn_bwd(B, Qd.ptr, sg.ptr, yg.ptr, pw.ptr, 1e-5, 0.5, p, mk.ptr if p > 0 else None, dAMd.ptr, dsd.ptr,
                           scale, dQ.ptr, part.ptr, dl2.ptr, stream())
    assert torch.equal(dl2.check(), dl.check())      # a second run: the same bits


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B", [1, 2])
def test_attention(B, p):
    g = torch.Generator().manual_seed(6)
    QKV = (2 * rnd(g, B, 65, 192)).requires_grad_(True)
    dO = rnd(g, B, 65, 64)
    Qd, dOd = Poisoned(QKV.detach().reshape(-1, 192).float()), Poisoned(dO.reshape(-1, 64).float())
    mk = Guarded(B * 16 * 65, 65, dtype=torch.uint8)
    Og = Guarded(B * 65, 64)
    L().vc_mhst_attn_fwd(B, Qd.ptr, 0.5, p, 4242, mk.ptr, Og.ptr, stream())
    keep = mk.check().double().reshape(B, 16, 65, 65)
    q, k, v = (QKV[:, :, 64 * i:64 * i + 64].reshape(B, 65, 16, 4).transpose(1, 2) for i in range(3))
    a = torch.softmax(q @ k.transpose(-1, -2) * 0.5, dim=-1) * keep / (1 - p)
    o = a @ v + torch.cat([torch.zeros_like(q[:, :, :1]), q[:, :, 1:]], dim=2)
    o = o.transpose(1, 2).reshape(B, 65, 64)
    o.backward(dO)
    close("vc_mhst_attn_fwd", (B, p), Og.check(), o.detach())
    if p == 0:
        assert bool((keep == 1).all())
        Og2 = Guarded(B * 65, 64)
        L().vc_mhst_attn_fwd(B, Qd.ptr, 0.5, 0.0, 0, None, Og2.ptr, stream())
        assert torch.equal(Og2.check(), Og.check())
    dQ = Guarded(B * 65, 192)
    L().vc_mhst_attn_bwd(B, Qd.ptr, 0.5, p, mk.ptr if p > 0 else None, dOd.ptr, dQ.ptr, stream())
    close("vc_mhst_attn_bwd", (B, p), dQ.check(), QKV.grad)


def test_attention_keep_fraction_and_ds_twin():
    B, p = 2, 0.1
    QKV = torch.zeros(B * 65, 192, device="cuda")
    n = B * 16 * 65 * 65
    seed = 987654321
    sd = torch.tensor([seed - 5], dtype=torch.int64, device="cuda")
    mk, mk2, Og = Guarded(B * 16 * 65, 65, dtype=torch.uint8), Guarded(B * 16 * 65, 65, dtype=torch.uint8), Guarded(B * 65, 64)
    L().vc_mhst_attn_fwd(B, QKV.data_ptr(), 0.5, p, seed, mk.ptr, Og.ptr, stream())
    L().vc_mhst_attn_fwd_ds(B, QKV.data_ptr(), 0.5, p, sd.data_ptr(), 5, mk2.ptr, Og.ptr, stream())
    keep = mk.check()
    assert torch.equal(keep, mk2.check())
    assert n >= 65536
    within("attention keep fraction", n, abs(float(keep.double().mean()) - (1 - p)), 5 * math.sqrt(p * (1 - p) / n))


@pytest.mark.parametrize("B,n", [(1, 12), (3, 16), (2, 70)])
def test_tail(B, n):
    g = torch.Generator().manual_seed(7)
    lg1, z = (3 * rnd(g, B, n)).requires_grad_(True), rnd(g, B, 64, 32).requires_grad_(True)
    W2, b2 = rnd(g, n, 32).requires_grad_(True), rnd(g, n).requires_grad_(True)
    cv, cc = rnd(g, 1).requires_grad_(True), rnd(g, 1).requires_grad_(True)
    dout = rnd(g, B, n)
    p1, p2 = torch.softmax(lg1, 1), torch.softmax(z.mean(1) @ W2.T + b2, 1)
    out = cv * p1 + cc * p2
    out.backward(dout)
    ldz = 35
    d = dict(lg1=Poisoned(lg1.detach().float()), z=Poisoned(z.detach().reshape(-1, 32).float(), ld=ldz),
             W2=Poisoned(W2.detach().float()), b2=Poisoned(b2.detach().reshape(1, -1).float(), lead=1),
             cv=Poisoned(cv.detach().reshape(1, 1).float(), lead=1), cc=Poisoned(cc.detach().reshape(1, 1).float(), lead=3),
             dout=Poisoned(dout.float()))
    p1g, p2g, avg, og = Guarded(B, n), Guarded(B, n), Guarded(B, 32), Guarded(B, n)
    L().vc_mhst_tail_fwd(B, n, d["lg1"].ptr, d["z"].ptr, ldz, d["W2"].ptr, d["b2"].ptr, d["cv"].ptr, d["cc"].ptr, p1g.ptr,
                         p2g.ptr, avg.ptr, og.ptr, stream())
    close("vc_mhst_tail_fwd", (B, n), og.check(), out.detach())
    close("vc_mhst_tail_fwd p1", (B, n), p1g.check(), p1.detach())
    close("vc_mhst_tail_fwd p2", (B, n), p2g.check(), p2.detach())
    dl, dz, part = Guarded(B, n), Guarded(B * 64, 32, ld=ldz), Guarded(B, n * 33 + 2)
    L().vc_mhst_tail_bwd(B, n, d["dout"].ptr, p1g.ptr, p2g.ptr, avg.ptr, d["W2"].ptr, d["cv"].ptr, d["cc"].ptr, dl.ptr,
                         dz.ptr, ldz, part.ptr, stream())
    close("vc_mhst_tail_bwd dlg1", (B, n), dl.check(), lg1.grad)
    close("vc_mhst_tail_bwd dz", (B, n), dz.check(), z.grad)
    p = part.check().double().sum(0)
    close("vc_mhst_tail_bwd dW2", (B, n), p[:n * 32], W2.grad)
    close("vc_mhst_tail_bwd db2", (B, n), p[n * 32:n * 33], b2.grad)
    close("vc_mhst_tail_bwd dcv dcc", (B, n), p[n * 33:], torch.cat([cv.grad, cc.grad]))
