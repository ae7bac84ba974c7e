"""The four hsiMamba row chains (vc_rowchain_front / _back / _back_bwd / _front_bwd, rowchain.hip) and
vc_rowchain_ln_params off the models' shapes, on the MI355X, against float64 torch on the CPU over the fp32 inputs
widened: row counts on both sides of every blocking decision (1, 15, 16, 17, 33 and 5088 on the 16-row kernels; 5089,
5103 and 5120 on the 32-row kernels, whose last block then holds 1, 15 and 32 rows), widths that are no multiple of
the 16-wide k chunk (4, 36, 72, 100: the zeroed Ts columns E .. kpad(E) - 1, block_gemm's min(n, N - 1) clamp, the
LayerNorm's col < E tail), more column tiles than waves (N2 = 260), a position period that does not divide the row
count, random permutations as scan orders with ndir in {1, 3, 10}, beta in {0 over NaN, 0.5, 1} on dx and on the
LayerNorm parameter gradients (adjacent and separate form, bit-identical).

Inputs are helpers.Poisoned (the chains take no leading dimensions: the NaN tail catches an over-read), every output
and the partial buffer (exactly vc_rowchain_ln_part_floats long) helpers.Guarded.  Bounds: 1e-5 of max |ref| on the
forward products, the LayerNorm outputs and statistics, 1e-4 on the gradients; LayerNorm rows of mean 1000 and unit
spread are held to 4 x torch fp32 CPU's deviation + 2 eps32 max |ref| (test_norm_layouts_gpu.rule).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import Guarded, Poisoned, rel_err, within
from test_kernels_gpu import rnd
from test_norm_layouts_gpu import max_dev, rule

gpu = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-6
SMALL_ROWS = [1, 15, 16, 17, 33]
LARGE_ROWS = [5088, 5089, 5103, 5120]      # 5088 = 159 x 32: the last count on the 16-row kernels


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


def cases(small_widths, large_widths):
    """(rows, widths, ordinal, regime): every small row count with every width triple, the large ones with the narrow
    triples; LayerNorm rows of unit scale everywhere, of mean 1000 at 17, 33 and 5103 rows"""
    out = [(r, w) for r in SMALL_ROWS for w in small_widths] + [(r, w) for r in LARGE_ROWS for w in large_widths]
    out = [(r, w, i) for i, (r, w) in enumerate(out)]
    return [c + ("unit",) for c in out] + [c + ("mean1000",) for c in out if c[0] in (17, 33, 5103)]


def ids(cs):
    return [f"r{r}-" + "x".join(map(str, w)) + "-" + regime for r, w, _, regime in cs]


def judge(name, shape, got, ref, bound, t32=None):
    """the fixed relative bound, or (mean-1000 rows, t32 = torch's fp32 result) section 17's rule on the max deviation"""
    if t32 is not None:
        within(name + " (mean 1000: max abs dev)", shape, max_dev(got, ref), rule(ref, t32), inclusive=True)
    else:
        within(name, shape, rel_err(got.numpy(), ref.numpy()), bound)


def ln_input_shift(regime):
    return 1000.0 if regime == "mean1000" else 0.0


# ------------------------------------------------------------------------------------------ front
def front_ref(x, w1, pos, lw, lb, w2, dtype):
    x, w1, pos, lw, lb, w2 = (t.to(dtype) for t in (x, w1, pos, lw, lb, w2))
    rows, Lp = x.shape[0], pos.shape[0]
    t = x @ w1.t() + pos[torch.arange(rows) % Lp]
    xn = F.layer_norm(t, (t.shape[1],), lw, lb, EPS)
    mu = t.mean(1)
    rs = torch.rsqrt(t.var(1, unbiased=False) + EPS)
    return t, xn, mu, rs, xn @ w2.t()


FRONT = cases([(4, 36, 260), (72, 100, 4), (144, 256, 36), (256, 100, 144), (100, 144, 72)], [(36, 36, 72), (72, 72, 36)])


@gpu
@pytest.mark.parametrize("rows,widths,i,regime", FRONT, ids=ids(FRONT))
def test_rowchain_front(L, rows, widths, i, regime):
    K0, E, N2 = widths
    Lp = (1, 7, 49)[i % 3]       # rows = 33 with Lp = 7 and the large counts with 7 / 49: rows % Lp != 0
    shape = f"rows={rows},K0={K0},E={E},N2={N2},L={Lp},{regime}"
    x, w1 = rnd(rows, K0, seed=1), rnd(E, K0, seed=2, scale=3.0 / math.sqrt(K0))
    pos = rnd(Lp, E, seed=3, scale=0.02) + ln_input_shift(regime)
    lw, lb, w2 = rnd(E, seed=4, scale=0.1) + 1.0, rnd(E, seed=5, scale=0.1), rnd(N2, E, seed=6, scale=1.0 / math.sqrt(E))
    ref = front_ref(x, w1, pos, lw, lb, w2, torch.float64)
    r32 = front_ref(x, w1, pos, lw, lb, w2, torch.float32) if regime == "mean1000" else [None] * 5
    ins = [Poisoned(t if t.dim() == 2 else t[None]) for t in (x, w1, pos, lw, lb, w2)]
    T, Xn, mu, rs, O = Guarded(rows, E), Guarded(rows, E), Guarded(1, rows), Guarded(1, rows), Guarded(rows, N2)
    assert L.vc_rowchain_front(rows, K0, E, N2, ins[0].ptr, ins[1].ptr, ins[2].ptr, Lp, T.ptr, ins[3].ptr, ins[4].ptr,
                               EPS, Xn.ptr, mu.ptr, rs.ptr, ins[5].ptr, O.ptr, S()) == 0
    judge("rowchain_front t", shape, T.check(), ref[0], 1e-5)
    judge("rowchain_front mean", shape, mu.check()[0], ref[2], 1e-5)
    judge("rowchain_front rstd", shape, rs.check()[0], ref[3], 1e-5, r32[3])
    judge("rowchain_front xn", shape, Xn.check(), ref[1], 1e-5, r32[1])
    judge("rowchain_front out", shape, O.check(), ref[4], 1e-5, r32[4])


# ------------------------------------------------------------------------------------------ back
BL = {1: (1, 1), 15: (3, 5), 16: (2, 8), 17: (1, 17), 33: (3, 11), 5088: (106, 48), 5089: (727, 7), 5103: (729, 7),
      5120: (80, 64)}


def back_ref(Y, inv, glog, xz, w1, res, lw, lb, w2, b2, B, Lq, dtype):
    Y, glog, xz, w1, res, lw, lb, w2, b2 = (t.to(dtype) for t in (Y, glog, xz, w1, res, lw, lb, w2, b2))
    ndir, D = inv.shape[0], Y.shape[1]
    gate = torch.softmax(glog, 0)
    Yk = Y.view(ndir, B, Lq, D)
    yp = sum(gate[k] * Yk[k][:, inv[k].long()] for k in range(ndir)).reshape(B * Lq, D)
    ys = yp * F.silu(xz[:, D:])
    t = ys @ w1.t() + res
    g = F.layer_norm(t, (t.shape[1],), lw, lb, EPS)
    return yp, ys, t, g, t.mean(1), torch.rsqrt(t.var(1, unbiased=False) + EPS), g @ w2.t() + b2


BACK = cases([(4, 36, 100), (72, 100, 260), (144, 256, 36), (256, 100, 144), (100, 144, 4)], [(36, 36, 72), (72, 72, 36)])


@gpu
@pytest.mark.parametrize("rows,widths,i,regime", BACK, ids=ids(BACK))
def test_rowchain_back(L, rows, widths, i, regime):
    D, E, N2 = widths
    B, Lq = BL[rows]
    ndir = (1, 3, 10)[i % 3]
    shape = f"B={B},L={Lq},D={D},E={E},N2={N2},ndir={ndir},{regime}"
    g = torch.Generator().manual_seed(100 + i)
    inv = torch.stack([torch.randperm(Lq, generator=g) for _ in range(ndir)]).int()
    glog, Y, xz = rnd(ndir, seed=11, scale=2.0), rnd(ndir * rows, D, seed=12), rnd(rows, 2 * D, seed=13, scale=2.0)
    w1 = rnd(E, D, seed=14, scale=6.0 / math.sqrt(D))
    res = rnd(rows, E, seed=15) + ln_input_shift(regime)
    lw, lb = rnd(E, seed=16, scale=0.1) + 1.0, rnd(E, seed=17, scale=0.1)
    w2, b2 = rnd(N2, E, seed=18, scale=1.0 / math.sqrt(E)), rnd(N2, seed=19, scale=0.1)
    ref = back_ref(Y, inv, glog, xz, w1, res, lw, lb, w2, b2, B, Lq, torch.float64)
    r32 = back_ref(Y, inv, glog, xz, w1, res, lw, lb, w2, b2, B, Lq, torch.float32) if regime == "mean1000" \
        else [None] * 7
    invd = inv.to(DEV)
    ins = [Poisoned(t if t.dim() == 2 else t[None]) for t in (glog, Y, xz, w1, res, lw, lb, w2, b2)]
    gl, Yp, xzp, w1p, resp, lwp, lbp, w2p, b2p = (t.ptr for t in ins)
    YP, YS, T2, G, O = Guarded(rows, D), Guarded(rows, D), Guarded(rows, E), Guarded(rows, E), Guarded(rows, N2)
    mu, rs = Guarded(1, rows), Guarded(1, rows)
    assert L.vc_rowchain_back(B, Lq, D, ndir, P(invd), gl, Yp, xzp, YP.ptr, YS.ptr, E, w1p, resp, T2.ptr, lwp, lbp, EPS,
                              G.ptr, mu.ptr, rs.ptr, N2, w2p, b2p, O.ptr, S()) == 0
    YP2, YS2 = Guarded(rows, D), Guarded(rows, D)
    assert L.vc_mamba_combine_fwd(B, Lq, D, ndir, P(invd), gl, Yp, xzp, YP2.ptr, YS2.ptr, S()) == 0
    yp, ys = YP.check(), YS.check()
    assert torch.equal(yp, YP2.check()) and torch.equal(ys, YS2.check())
    judge("rowchain_back ypsum", shape, yp, ref[0], 1e-5)
    judge("rowchain_back ysum", shape, ys, ref[1], 1e-5)
    judge("rowchain_back t2", shape, T2.check(), ref[2], 1e-5)
    judge("rowchain_back mean", shape, mu.check()[0], ref[4], 1e-5)
    judge("rowchain_back rstd", shape, rs.check()[0], ref[5], 1e-5, r32[5])
    judge("rowchain_back g", shape, G.check(), ref[3], 1e-5, r32[3])
    judge("rowchain_back out", shape, O.check(), ref[6], 1e-5, r32[6])


# ------------------------------------------------------------------------------------------ backward chains
def ln_grads(dg, t, lw, dtype):
    """(dt, dw, db) of LayerNorm(t) under the output gradient dg, by autograd in dtype"""
    tr, wr = t.to(dtype).clone().requires_grad_(True), lw.to(dtype).clone().requires_grad_(True)
    br = torch.zeros_like(wr).requires_grad_(True)
    F.layer_norm(tr, (t.shape[1],), wr, br, EPS).backward(dg)
    return tr.grad, wr.grad, br.grad


def stats32(t):
    t = t.double()
    return t.mean(1).float(), torch.rsqrt(t.var(1, unbiased=False) + EPS).float()


def check_ln_params(L, tag, shape, rows, E, part, dw_ref, db_ref, dw32, db32):
    """vc_rowchain_ln_params at beta 0 (over NaN), 0.5 and 1, adjacent (db == dw + E) and separate, bit-identical"""
    p0 = rnd(2 * E, seed=77)
    for beta in (0.0, 0.5, 1.0):
        both = Guarded(1, 2 * E, init=p0 if beta else None)
        gw, gb = Guarded(1, E, init=p0[:E] if beta else None), Guarded(1, E, init=p0[E:] if beta else None)
        assert L.vc_rowchain_ln_params(rows, E, part.ptr, both.ptr, both.ptr + 4 * E, beta, S()) == 0
        assert L.vc_rowchain_ln_params(rows, E, part.ptr, gw.ptr, gb.ptr, beta, S()) == 0
        adj, w, b = both.check()[0], gw.check()[0], gb.check()[0]
        assert torch.equal(adj[:E], w) and torch.equal(adj[E:], b), beta
        judge(f"{tag} ln_params dw beta={beta}", shape, w, dw_ref + beta * p0[:E].double(), 1e-4,
              None if dw32 is None else dw32 + beta * p0[:E])
        judge(f"{tag} ln_params db beta={beta}", shape, b, db_ref + beta * p0[E:].double(), 1e-4,
              None if db32 is None else db32 + beta * p0[E:])
    part.check()


def back_bwd_ref(dcd, wcd, t2, lw, wout, xz, yp, dtype):
    dcd, wcd, wout, xz, yp = (t.to(dtype) for t in (dcd, wcd, wout, xz, yp))
    D = yp.shape[1]
    dt, dw, db = ln_grads(dcd @ wcd, t2, lw, dtype)
    dys = dt @ wout
    z = xz[:, D:]
    sg = torch.sigmoid(z)
    return dt, dys * z * sg, dys * yp * sg * (1 + z * (1 - sg)), dw, db


BACK_BWD = cases([(4, 36, 72), (100, 100, 36), (256, 36, 144), (72, 144, 100), (144, 256, 4)], [(36, 36, 72), (72, 72, 36)])


@gpu
@pytest.mark.parametrize("rows,widths,i,regime", BACK_BWD, ids=ids(BACK_BWD))
def test_rowchain_back_bwd(L, rows, widths, i, regime):
    Cout, E, D = widths
    shape = f"rows={rows},Cout={Cout},E={E},D={D},{regime}"
    dcd, wcd = rnd(rows, Cout, seed=21), rnd(Cout, E, seed=22, scale=1.0 / math.sqrt(Cout))
    t2 = rnd(rows, E, seed=23, scale=3.0 ** 0.5) + 0.5 + ln_input_shift(regime)
    lw, wout = rnd(E, seed=24, scale=0.1) + 1.0, rnd(E, D, seed=25, scale=1.0 / math.sqrt(E))
    xz, yp = rnd(rows, 2 * D, seed=26, scale=2.0), rnd(rows, D, seed=27)
    ref = back_bwd_ref(dcd, wcd, t2, lw, wout, xz, yp, torch.float64)
    r32 = back_bwd_ref(dcd, wcd, t2, lw, wout, xz, yp, torch.float32) if regime == "mean1000" else [None] * 5
    mu, rs = stats32(t2)
    ins = [Poisoned(t if t.dim() == 2 else t[None]) for t in (dcd, wcd, t2, mu, rs, lw, wout, xz, yp)]
    dT, dYP, dXZ = Guarded(rows, E), Guarded(rows, D), Guarded(rows, 2 * D)
    part = Guarded(1, L.vc_rowchain_ln_part_floats(rows, E))
    assert L.vc_rowchain_back_bwd(rows, Cout, E, D, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, ins[4].ptr,
                                  ins[5].ptr, dT.ptr, part.ptr, ins[6].ptr, ins[7].ptr, ins[8].ptr, dYP.ptr, dXZ.ptr,
                                  S()) == 0
    judge("rowchain_back_bwd dt", shape, dT.check(), ref[0], 1e-4, r32[0])
    judge("rowchain_back_bwd dyp", shape, dYP.check(), ref[1], 1e-4, r32[1])
    dxz = dXZ.check()
    judge("rowchain_back_bwd dz", shape, dxz[:, D:], ref[2], 1e-4, r32[2])
    assert torch.isnan(dxz[:, :D]).all()       # the x half is the scan backward's
    check_ln_params(L, "rowchain_back_bwd", shape, rows, E, part, ref[3], ref[4], r32[3], r32[4])


def front_bwd_ref(dxz, win, t, lw, res, wpe, dtype):
    dxz, win, res, wpe = (x.to(dtype) for x in (dxz, win, res, wpe))
    dl, dw, db = ln_grads(dxz @ win, t, lw, dtype)
    dtt = dl + res
    return dtt, dtt @ wpe, dw, db


# (K0, E, Cin): K0 and E multiples of 4 (the float4 staging of dxz and of the LN rows), any Cin
FRONT_BWD = cases([(4, 36, 1), (72, 100, 3), (144, 256, 63), (256, 100, 144), (100, 144, 3)], [(36, 36, 63), (72, 72, 3)])


@gpu
@pytest.mark.parametrize("rows,widths,i,regime", FRONT_BWD, ids=ids(FRONT_BWD))
def test_rowchain_front_bwd(L, rows, widths, i, regime):
    K0, E, Cin = widths
    shape = f"rows={rows},K0={K0},E={E},Cin={Cin},{regime}"
    dxz, win = rnd(rows, K0, seed=31), rnd(K0, E, seed=32, scale=1.0 / math.sqrt(K0))
    t = rnd(rows, E, seed=33, scale=3.0 ** 0.5) - 0.3 + ln_input_shift(regime)
    lw, res = rnd(E, seed=34, scale=0.1) + 1.0, rnd(rows, E, seed=35)
    wpe = rnd(E, Cin, seed=36, scale=1.0 / math.sqrt(E))
    dx0, dxa = rnd(rows, Cin, seed=37), rnd(rows, Cin, seed=38)
    ref = front_bwd_ref(dxz, win, t, lw, res, wpe, torch.float64)
    r32 = front_bwd_ref(dxz, win, t, lw, res, wpe, torch.float32) if regime == "mean1000" else [None] * 4
    mu, rs = stats32(t)
    ins = [Poisoned(x if x.dim() == 2 else x[None]) for x in (dxz, win, t, mu, rs, lw, res, wpe, dxa)]
    outs = []
    # (dx given, beta, dx_add given): every beta with and without the addend, and no dx at all
    for with_dx, beta, with_add in [(True, 0.0, False), (True, 0.5, True), (True, 1.0, False), (True, 0.0, True),
                                    (False, 1.0, False)]:
        dTt = Guarded(rows, E)
        dX = Guarded(rows, Cin, init=dx0 if (beta or not with_dx) else None)
        part = Guarded(1, L.vc_rowchain_ln_part_floats(rows, E))
        assert L.vc_rowchain_front_bwd(rows, K0, E, Cin, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, ins[4].ptr,
                                       ins[5].ptr, ins[6].ptr, dTt.ptr, part.ptr, ins[7].ptr,
                                       dX.ptr if with_dx else None, beta, ins[8].ptr if with_add else None, S()) == 0
        tag = f"rowchain_front_bwd[dx={int(with_dx)},beta={beta},add={int(with_add)}]"
        got = dTt.check()
        judge(tag + " dtt", shape, got, ref[0], 1e-4, r32[0])
        outs.append((got, part.check()))
        if with_dx:
            extra = beta * dx0.double() + (dxa.double() if with_add else 0.0)
            judge(tag + " dx", shape, dX.check(), ref[1] + extra, 1e-4, None if r32[1] is None else r32[1] + extra.float())
        else:
            assert torch.equal(dX.check(), dx0)
    for o in outs[1:]:       # dtt and the partials do not depend on what is done with dx
        assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1])
    check_ln_params(L, "rowchain_front_bwd", shape, rows, E, part, ref[2], ref[3], r32[2], r32[3])
