"""The spatial kernels off the models' shapes, on the MI355X, against float64 torch on the CPU over the fp32 inputs
widened: the implicit-GEMM 3x3 convolutions of conv_gemm.hip (vc_conv3x3_fwd / _wgrad / _dgrad), the tap-major ones of
conv_tap.hip (vc_conv3x3_tap_fwd / _wgrad / _wgrad_oihw / _dgrad with vc_conv3x3_pack), and conv.hip's 2x2 max pool
(vc_maxpool2_fwd / _bwd), im2col / col2im (vc_im2col3x3, vc_col2im3x3) and vc_bn_im2col3x3.

Maps with H != W (the kernels divide by OW, OH, W and H separately: a swap of two divisors is invisible on a square map),
one output row, channel counts that leave a k tail, O just past one tile, a 9 C that makes the bias gradient's ones
column open a tile column of its own; every leading dimension natural, + 4 and + 3; a weight / dy base one float off
16 B (the scalar staging); ReLU and no ReLU, bias / BatchNorm affine / dbias present and null, beta in {0 over NaN,
0.5, 1}; no workspace, one of 2 M Ne + 5 floats (the split-count clamp acts; its tail is guarded) and a large one.  The
full cross is trimmed: per (geometry, layout) a fixed list of option tuples runs, chosen so that every value of every
option meets the unsplit kernel (no workspace) and the split one (a workspace, on the geometries whose K allows a
split).  Integer-valued inputs (exact_conv: every partial sum an integer below 2^24, asserted on the CPU also without a
GPU) must give torch.equal whatever the split.

Inputs are helpers.Poisoned, outputs and tight workspaces helpers.Guarded.  For the tap convolutions only
(include/vitcnn.h), where C % 4 != 0 and ldx % 4 == 0 the row padding up to C rounded to 4 holds finite garbage (it is
read against zero weights); every other gap holds NaN.  Bounds: 1e-5 of max |ref| (conv_gemm, im2col with the affine,
col2im, vc_bn_im2col3x3), the two formulas of tests/test_conv_tap_gpu.py for the tap convolutions, torch.equal for the
pool, the packs, the plain im2col copy and every bit-identity claim.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import Guarded, Poisoned, rel_err, within
from test_kernels_gpu import rnd

gpu = pytest.mark.gpu
DEV = "cuda"

# (B, H, W, C, O, pad)
GEOS = [
    (2, 5, 9, 5, 7, 0),
    (2, 9, 5, 5, 7, 1),
    (1, 3, 4, 1, 1, 0),        # one output row
    (3, 7, 6, 33, 20, 1),      # K = 9 C = 297: a k tail of 9 (and, with a workspace, a split forward)
    (2, 6, 7, 64, 65, 0),      # 9 C = 576: the ones column opens a tile column of its own; O just past one tile
    (2, 4, 5, 132, 64, 1),     # K = 1188 >= 8 BK on few tiles: the forward and the data gradient split
    (4, 9, 11, 5, 7, 1),       # 396 output pixels: the weight gradient (K = pixels) splits
]
GIDS = ["x".join(map(str, g)) for g in GEOS]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vitcnn_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def big():
    return torch.empty(1 << 22, device=DEV)


def S():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return t.data_ptr() if t is not None else None


def up4(n):
    return -(-n // 4) * 4


def ints(*shape, seed=0, lo=-4, hi=4, even=False):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi + 1, shape, generator=g).float()
    return 2 * torch.div(t, 2, rounding_mode="trunc") if even else t


def out_hw(H, W, pad):
    return H + 2 * pad - 2, W + 2 * pad - 2


@functools.lru_cache(maxsize=None)
def conv_data(geo, exact=False):
    """x [B H W, C], w [O, C, 3, 3], bias [O], the BatchNorm (mean, invstd, weight, bias) [C] each, dy [B OH OW, O]"""
    B, H, W, C, O, pad = geo
    OH, OW = out_hw(H, W, pad)
    if exact:     # integers; the affine's scale invstd w is a power of two, so (x - mean) sc + b stays an integer
        bn = (ints(C, seed=5), torch.full((C,), 0.5), 2.0 * (1.0 + ints(C, seed=6, lo=0, hi=1)), ints(C, seed=7))
        return ints(B * H * W, C, seed=1), ints(O, C, 3, 3, seed=2), ints(O, seed=3, lo=-8, hi=8), bn, \
            ints(B * OH * OW, O, seed=4)
    bn = (rnd(C, seed=5), rnd(C, seed=6).abs() + 0.5, rnd(C, seed=7).abs() + 0.5, rnd(C, seed=8))
    return rnd(B * H * W, C, seed=1), rnd(O, C, 3, 3, seed=2, scale=(3.0 / (9 * C)) ** 0.5), rnd(O, seed=3), bn, \
        rnd(B * OH * OW, O, seed=4)


@functools.lru_cache(maxsize=None)
def conv_ref(geo, with_bn, exact=False):
    """float64: (y before bias and ReLU [M, O], dw [O, 9C], db [O], dx with respect to the post-affine input [B H W, C])"""
    B, H, W, C, O, pad = geo
    x, w, _, bn, dy = conv_data(geo, exact)
    x64 = x.double()
    if with_bn:
        mean, inv, g, b = (t.double() for t in bn)
        x64 = (x64 - mean) * (inv * g) + b
    xin = x64.view(B, H, W, C).permute(0, 3, 1, 2).clone().requires_grad_(True)
    wr = w.double().clone().requires_grad_(True)
    y = F.conv2d(xin, wr, None, padding=pad)
    OH, OW = out_hw(H, W, pad)
    y.backward(dy.double().view(B, OH, OW, O).permute(0, 3, 1, 2))
    return (y.detach().permute(0, 2, 3, 1).reshape(-1, O), wr.grad.reshape(O, 9 * C), dy.double().sum(0),
            xin.grad.permute(0, 2, 3, 1).reshape(-1, C))


def workspace(kind, n_tight, big):
    """(pointer, floats, the Guarded buffer to check or None): no workspace, 2 M Ne + 5 floats, or the large one"""
    if kind is None:
        return None, 0, None
    if kind == "big":
        return P(big), big.numel(), None
    g = Guarded(1, n_tight)
    return g.ptr, n_tight, g


# ------------------------------------------------------------------------------------------ conv_gemm.hip
# name -> (leading dimension of a natural width, lead of the weight (fwd, dgrad) / dy (wgrad))
GEMM_LAYOUTS = {"nat": (lambda w: w, 0), "pad4": (lambda w: w + 4, 0), "pad3": (lambda w: w + 3, 0),
                "lead1": (up4, 1)}        # lead1: the leading dimensions would allow vectors, the base does not
# (relu, bias, BatchNorm affine, workspace): every value of every option with and without a workspace
FWD_OPTS = [(1, True, True, "big"), (0, False, False, "big"), (0, True, False, "tight"), (1, False, True, "tight"),
            (1, True, False, None), (0, False, True, None)]
# (beta, dbias, BatchNorm affine, workspace)
WGRAD_OPTS = [(0.0, True, True, "big"), (0.5, False, False, "big"), (1.0, True, False, "tight"),
              (0.5, True, True, "tight"), (0.0, False, True, None), (1.0, True, False, None), (0.5, True, True, None)]
# (beta, workspace)
DGRAD_OPTS = [(0.0, None), (0.5, None), (1.0, None), (0.0, "big"), (0.5, "tight"), (1.0, "big")]


def bn_ptrs(bn, on):
    dev = [t.to(DEV) for t in bn] if on else [None] * 4
    return dev, [P(t) for t in dev]


def gemm_fwd(L, geo, layout, opts, big, exact=False):
    B, H, W, C, O, pad = geo
    ld, lead = GEMM_LAYOUTS[layout]
    relu, with_bias, with_bn, ws_kind = opts
    x, w, bias, bn, _ = conv_data(geo, exact)
    OH, OW = out_hw(H, W, pad)
    M = B * OH * OW
    ref = conv_ref(geo, with_bn, exact)[0] + (bias.double() if with_bias else 0.0)
    ref = torch.relu(ref) if relu else ref
    xp, wp = Poisoned(x, ld=ld(C)), Poisoned(w.reshape(O, 9 * C), lead=lead)
    keep, bp = bn_ptrs(bn, with_bn)
    bd = bias.to(DEV) if with_bias else None
    y = Guarded(M, O, ld=ld(O))
    wsp, wsn, tight = workspace(ws_kind, 2 * M * O + 5, big)
    assert L.vc_conv3x3_fwd(B, H, W, C, O, pad, xp.ptr, xp.ld, *bp, wp.ptr, P(bd), relu, y.ptr, y.ld, wsp, wsn, S()) == 0
    got = y.check()
    if tight is not None:
        tight.check()
    return got, ref


def gemm_wgrad(L, geo, layout, opts, big, exact=False):
    B, H, W, C, O, pad = geo
    ld, lead = GEMM_LAYOUTS[layout]
    beta, with_db, with_bn, ws_kind = opts
    x, _, _, bn, dy = conv_data(geo, exact)
    dw0 = ints(O, 9 * C, seed=11, lo=-8, hi=8, even=True) if exact else rnd(O, 9 * C, seed=11)
    db0 = ints(O, seed=12, lo=-8, hi=8, even=True) if exact else rnd(O, seed=12)
    _, dw_ref, db_ref, _ = conv_ref(geo, with_bn, exact)
    xp, dyp = Poisoned(x, ld=ld(C)), Poisoned(dy, ld=ld(O), lead=lead)
    keep, bp = bn_ptrs(bn, with_bn)
    dw = Guarded(O, 9 * C, init=dw0 if beta else None)
    db = Guarded(1, O, init=db0 if beta else None)
    Ne = 9 * C + int(with_db)
    wsp, wsn, tight = workspace(ws_kind, 2 * O * Ne + 5, big)
    assert L.vc_conv3x3_wgrad(B, H, W, C, O, pad, xp.ptr, xp.ld, *bp, dyp.ptr, dyp.ld, beta, dw.ptr,
                              db.ptr if with_db else None, wsp, wsn, S()) == 0
    got_w, got_b = dw.check(), db.check()[0]
    if tight is not None:
        tight.check()
    if not with_db:       # not passed: as it was
        assert torch.equal(got_b, db0) if beta else bool(torch.isnan(got_b).all())
    return got_w, dw_ref + beta * dw0.double(), (got_b if with_db else None), db_ref + beta * db0.double()


def gemm_dgrad(L, geo, layout, opts, big, exact=False):
    B, H, W, C, O, pad = geo
    ld, lead = GEMM_LAYOUTS[layout]
    beta, ws_kind = opts
    _, w, _, _, dy = conv_data(geo, exact)
    dx0 = ints(B * H * W, C, seed=13, lo=-8, hi=8, even=True) if exact else rnd(B * H * W, C, seed=13)
    ref = conv_ref(geo, False, exact)[3] + beta * dx0.double()
    dyp, wp = Poisoned(dy, ld=ld(O)), Poisoned(w.reshape(O, 9 * C), lead=lead)
    dx = Guarded(B * H * W, C, ld=ld(C), init=dx0 if beta else None)
    wsp, wsn, tight = workspace(ws_kind, 2 * B * H * W * C + 5, big)
    assert L.vc_conv3x3_dgrad(B, H, W, C, O, pad, dyp.ptr, dyp.ld, wp.ptr, beta, dx.ptr, dx.ld, wsp, wsn, S()) == 0
    got = dx.check()
    if tight is not None:
        tight.check()
    return got, ref


@gpu
@pytest.mark.parametrize("layout", list(GEMM_LAYOUTS))
@pytest.mark.parametrize("geo", GEOS, ids=GIDS)
def test_conv3x3_fwd(L, big, geo, layout):
    for opts in FWD_OPTS:
        got, ref = gemm_fwd(L, geo, layout, opts, big)
        within("conv3x3_fwd", f"{geo} {layout} relu={opts[0]} bias={int(opts[1])} bn={int(opts[2])} ws={opts[3]}",
               rel_err(got.numpy(), ref.numpy()), 1e-5)
        if got.numel() >= 64:       # both branches of the ReLU / no clamp without it
            assert (bool((got == 0).any()) and bool((got > 0).any())) if opts[0] else bool((got < 0).any())


@gpu
@pytest.mark.parametrize("layout", list(GEMM_LAYOUTS))
@pytest.mark.parametrize("geo", GEOS, ids=GIDS)
def test_conv3x3_wgrad(L, big, geo, layout):
    for opts in WGRAD_OPTS:
        got_w, ref_w, got_b, ref_b = gemm_wgrad(L, geo, layout, opts, big)
        shape = f"{geo} {layout} beta={opts[0]} dbias={int(opts[1])} bn={int(opts[2])} ws={opts[3]}"
        within("conv3x3_wgrad dweight", shape, rel_err(got_w.numpy(), ref_w.numpy()), 1e-5)
        if got_b is not None:
            within("conv3x3_wgrad dbias", shape, rel_err(got_b.numpy(), ref_b.numpy()), 1e-5)


@gpu
@pytest.mark.parametrize("layout", list(GEMM_LAYOUTS))
@pytest.mark.parametrize("geo", GEOS, ids=GIDS)
def test_conv3x3_dgrad(L, big, geo, layout):
    for opts in DGRAD_OPTS:
        got, ref = gemm_dgrad(L, geo, layout, opts, big)
        within("conv3x3_dgrad", f"{geo} {layout} beta={opts[0]} ws={opts[1]}", rel_err(got.numpy(), ref.numpy()), 1e-5)


EXACT_GEOS = [GEOS[0], GEOS[1], GEOS[4], GEOS[5], GEOS[6]]


def exact_conv(geo):
    """no GPU needed: on the integer inputs every reference is integer-valued and every partial sum, in any order, an
    integer below 2^24 (sum |a| |b| < 2^24, the accumulated-into values even where beta = 0.5), so fp32 accumulates
    without rounding and the kernels must return the float64 reference bit for bit, split or not"""
    B, H, W, C, O, pad = geo
    x, w, bias, bn, dy = conv_data(geo, True)
    for with_bn in (False, True):
        xa = x.double()
        if with_bn:
            xa = (xa - bn[0].double()) * (bn[1] * bn[2]).double() + bn[3].double()
            assert torch.equal(xa, xa.round()) and torch.equal(xa.float().double(), xa)
        worst = 9 * C * float(xa.abs().max()) * float(w.abs().max()) + 8              # fwd: K = 9 C terms + bias
        worst = max(worst, dy.shape[0] * float(dy.abs().max()) * max(float(xa.abs().max()), 1.0) + 8)   # wgrad, dbias
        worst = max(worst, 9 * O * float(dy.abs().max()) * float(w.abs().max()) + 8)  # dgrad
        assert worst < 2 ** 24
        for r in conv_ref(geo, with_bn, True):
            assert torch.equal(r, r.round()) and float(r.abs().max()) < 2 ** 24 - 8


def test_exact_conv_generators_are_exact():
    for geo in EXACT_GEOS:
        exact_conv(geo)


@gpu
@pytest.mark.parametrize("geo", EXACT_GEOS, ids=["x".join(map(str, g)) for g in EXACT_GEOS])
def test_conv3x3_exact(L, big, geo):
    """integer data: a dropped, duplicated or misplaced k element, pixel or bias cannot hide in a tolerance; layout i
    runs with the i-th option tuple and the next two (every option tuple on at least one layout)"""
    exact_conv(geo)
    for i, layout in enumerate(GEMM_LAYOUTS):
        for j in range(3):
            opts = FWD_OPTS[(i + 2 * j) % len(FWD_OPTS)]
            got, ref = gemm_fwd(L, geo, layout, opts, big, True)
            assert torch.equal(got.double(), ref), ("fwd", layout, opts)
            opts = WGRAD_OPTS[(2 * i + j) % len(WGRAD_OPTS)]
            got_w, ref_w, got_b, ref_b = gemm_wgrad(L, geo, layout, opts, big, True)
            assert torch.equal(got_w.double(), ref_w), ("wgrad", layout, opts)
            assert got_b is None or torch.equal(got_b.double(), ref_b), ("dbias", layout, opts)
            opts = DGRAD_OPTS[(i + 2 * j) % len(DGRAD_OPTS)]
            got, ref = gemm_dgrad(L, geo, layout, opts, big, True)
            assert torch.equal(got.double(), ref), ("dgrad", layout, opts)


# ------------------------------------------------------------------------------------------ conv_tap.hip
TAP_GEOS = GEOS + [(4, 11, 9, 8, 20, 1)]     # + a pipelined weight gradient (O % 4 == 0) with 396 pixels: it splits
TAP_IDS = ["x".join(map(str, g)) for g in TAP_GEOS]
# name -> (ldx, lead x, lddy, lead dy, ldy, lddx) from (C, O); "al" keeps the pipelined kernel where O % 4 == 0
TAP_LAYOUTS = {
    "nat": lambda C, O: (C, 0, O, 0, O, C),
    "al": lambda C, O: (up4(C) + 4, 0, up4(O) + 4, 0, up4(O) + 4, up4(C) + 4),
    "x1": lambda C, O: (up4(C) + 4, 1, up4(O) + 4, 0, up4(O) + 4, up4(C) + 4),      # fallback: x off 16 B
    "dy1": lambda C, O: (up4(C) + 4, 0, up4(O) + 4, 1, up4(O) + 4, up4(C) + 4),     # fallback: dy off 16 B
    "odd": lambda C, O: (up4(C) + 4, 0, O + 3, 0, O + 5, C + 5),                    # fallback: lddy odd
}
TAP_WS = [None, "tight", "lead1"]


def tap_x(x, ldx, lead):
    """the tap convolutions' input: NaN poison, but finite garbage in the columns C .. C rounded to 4 where
    C % 4 != 0 and ldx % 4 == 0 (include/vitcnn.h: read against zero weights)"""
    p = Poisoned(x, ld=ldx, lead=lead)
    C = x.shape[1]
    if C % 4 and ldx % 4 == 0:
        p.flat.as_strided((x.shape[0], up4(C) - C), (ldx, 1), lead + C).fill_(3.0)
    return p


def tap_workspace(kind, slab):
    """no workspace; 2 slabs + 5 floats (the clamp acts); 4 slabs + 3 floats one float off 16 B (scalar combine)"""
    if kind is None:
        return None, 0, None
    g = Guarded(1, 2 * slab + 5) if kind == "tight" else Guarded(1, 4 * slab + 3, lead=1)
    return g.ptr, g.C, g


def tap_bounds(name, shape, got, ref, C, O):
    got, ref = got.double(), ref.double()
    within(name + " max", shape, float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30)),
           2e-6 * (9 * max(C, O)) ** 0.5)
    within(name + " norm", shape, float((got - ref).norm() / max(float(ref.norm()), 1e-30)), 3e-6)


@gpu
@pytest.mark.parametrize("geo", TAP_GEOS, ids=TAP_IDS)
def test_conv3x3_pack(L, geo):
    """modes 0 (Wt [O][9][Cw], padding written 0), 1 (W2 [9][O][C]) and 2 (back to the torch layout): copies"""
    _, _, _, C, O, _ = geo
    w = conv_data(geo)[1]
    Cw = up4(C)
    wp = Poisoned(w.reshape(O, 9 * C))
    wt, w2, back = Guarded(O, 9 * Cw), Guarded(9 * O, C), Guarded(O, 9 * C)
    assert L.vc_conv3x3_pack(O, C, 0, wp.ptr, wt.ptr, 0.0, S()) == 0
    assert L.vc_conv3x3_pack(O, C, 1, wp.ptr, w2.ptr, 0.0, S()) == 0
    wt_ref = torch.zeros(O, 9, Cw)
    wt_ref[:, :, :C] = w.permute(0, 2, 3, 1).reshape(O, 9, C)
    assert torch.equal(wt.check().view(O, 9, Cw), wt_ref)
    assert torch.equal(w2.check().view(9, O, C), w.permute(2, 3, 0, 1).reshape(9, O, C))
    dwt = Poisoned(w.permute(0, 2, 3, 1).reshape(O, 9 * C).contiguous())
    assert L.vc_conv3x3_pack(O, C, 2, dwt.ptr, back.ptr, 0.0, S()) == 0
    assert torch.equal(back.check().view(O, C, 3, 3), w)


def packed(L, geo):
    """Wt on the device (vc_conv3x3_pack mode 0, checked by test_conv3x3_pack), NaN-tailed"""
    _, _, _, C, O, _ = geo
    wp = Poisoned(conv_data(geo)[1].reshape(O, 9 * C))
    wt = Guarded(O, 9 * up4(C))
    assert L.vc_conv3x3_pack(O, C, 0, wp.ptr, wt.ptr, 0.0, S()) == 0
    torch.cuda.synchronize()
    wt.flat[wt.span:] = float("nan")       # an input from here on: an over-read must show
    return wt


@gpu
@pytest.mark.parametrize("layout", list(TAP_LAYOUTS))
@pytest.mark.parametrize("geo", TAP_GEOS, ids=TAP_IDS)
def test_conv3x3_tap_fwd_dgrad(L, geo, layout):
    B, H, W, C, O, pad = geo
    ldx, leadx, lddy, leaddy, ldy, lddx = TAP_LAYOUTS[layout](C, O)
    x, _, bias, _, dy = conv_data(geo)
    OH, OW = out_hw(H, W, pad)
    M, Min = B * OH * OW, B * H * W
    y_ref, _, _, dx_ref = conv_ref(geo, False)
    dx0 = rnd(Min, C, seed=13)
    wt = packed(L, geo)
    xp, dyp, bd = tap_x(x, ldx, leadx), Poisoned(dy, ld=lddy, lead=leaddy), bias.to(DEV)
    for i, kind in enumerate(TAP_WS):
        with_bias, beta = i != 1, (0.0, 0.5, 0.0)[i]
        shape = f"{geo} {layout} ws={kind}"
        y = Guarded(M, O, ld=ldy)
        wsp, wsn, g = tap_workspace(kind, M * O)
        assert L.vc_conv3x3_tap_fwd(B, H, W, C, O, pad, xp.ptr, ldx, wt.ptr, P(bd) if with_bias else None, y.ptr, ldy,
                                    wsp, wsn, S()) == 0
        tap_bounds("conv3x3_tap_fwd", shape, y.check(), y_ref + (bias.double() if with_bias else 0.0), C, O)
        if g is not None:
            g.check()
        dx = Guarded(Min, C, ld=lddx, init=dx0 if beta else None)
        wsp, wsn, g = tap_workspace(kind, Min * C)
        assert L.vc_conv3x3_tap_dgrad(B, H, W, C, O, pad, dyp.ptr, lddy, wt.ptr, beta, dx.ptr, lddx, wsp, wsn, S()) == 0
        tap_bounds("conv3x3_tap_dgrad", shape + f" beta={beta}", dx.check(), dx_ref + beta * dx0.double(), C, O)
        if g is not None:
            g.check()


@gpu
@pytest.mark.parametrize("layout", list(TAP_LAYOUTS))
@pytest.mark.parametrize("geo", TAP_GEOS, ids=TAP_IDS)
def test_conv3x3_tap_wgrad(L, geo, layout):
    """vc_conv3x3_tap_wgrad and _wgrad_oihw (db null and present) per workspace; _wgrad_oihw without db is bit-identical
    to _wgrad + pack mode 2 under the same workspace, with db (slabs one column wider: another split count under a
    tight workspace) without a workspace and under the roomy one"""
    B, H, W, C, O, pad = geo
    ldx, leadx, lddy, leaddy, _, _ = TAP_LAYOUTS[layout](C, O)
    x, _, _, _, dy = conv_data(geo)
    OH, OW = out_hw(H, W, pad)
    _, dw_ref, db_ref, _ = conv_ref(geo, False)
    dw_ref = dw_ref.view(O, C, 3, 3)
    xp, dyp = tap_x(x, ldx, leadx), Poisoned(dy, ld=lddy, lead=leaddy)
    for kind in TAP_WS:
        shape = f"{geo} {layout} ws={kind}"
        dwt, dw = Guarded(O, 9 * C), Guarded(O, 9 * C)
        wsp, wsn, g = tap_workspace(kind, O * 9 * C)
        assert L.vc_conv3x3_tap_wgrad(B, H, W, C, O, pad, xp.ptr, ldx, dyp.ptr, lddy, dwt.ptr, wsp, wsn, S()) == 0
        dwt.check()
        assert L.vc_conv3x3_pack(O, C, 2, dwt.ptr, dw.ptr, 0.0, S()) == 0
        two = dw.check().view(O, C, 3, 3)
        tap_bounds("conv3x3_tap_wgrad", shape, two, dw_ref, C, O)
        d2 = Guarded(O, 9 * C)
        assert L.vc_conv3x3_tap_wgrad_oihw(B, H, W, C, O, pad, xp.ptr, ldx, dyp.ptr, lddy, d2.ptr, None, wsp, wsn,
                                           S()) == 0
        assert torch.equal(d2.check().view(O, C, 3, 3), two)
        if g is not None:
            g.check()
        d3, db = Guarded(O, 9 * C), Guarded(1, O)
        wsp, wsn, g = tap_workspace(kind, O * (9 * C + 1))
        assert L.vc_conv3x3_tap_wgrad_oihw(B, H, W, C, O, pad, xp.ptr, ldx, dyp.ptr, lddy, d3.ptr, db.ptr, wsp, wsn,
                                           S()) == 0
        got3 = d3.check().view(O, C, 3, 3)
        if kind != "tight":
            assert torch.equal(got3, two)
        tap_bounds("conv3x3_tap_wgrad_oihw", shape, got3, dw_ref, C, O)
        within("conv3x3_tap_wgrad_oihw db", shape, rel_err(db.check()[0].numpy(), db_ref.numpy()),
               2e-6 * (B * OH * OW) ** 0.5)
        if g is not None:
            g.check()


# ------------------------------------------------------------------------------------------ conv.hip: max pool
POOLS = [(2, 2, 2, 1), (2, 5, 8, 3), (3, 9, 4, 70), (1, 3, 3, 64), (2, 7, 11, 130)]


@functools.lru_cache(maxsize=None)
def pool_case(B, H, W, C):
    """input with tied windows (window (0, 0) of element 0: four equal rows; its last window of the first row: taps 1
    and 3 equal and largest; window (1, 0) where it exists: taps 2 and 3) and one NaN (tap 2 of window (0, 0) of the
    last element); float64 max_pool2d with indices and its autograd"""
    PH, PW = H // 2, W // 2
    x = rnd(B, H, W, C, seed=91)
    x[0, 0, 1] = x[0, 1, 0] = x[0, 1, 1] = x[0, 0, 0]
    if PW > 1:
        x[0, 0, 2 * PW - 1] = x[0, 1, 2 * PW - 1] = x[0, 0, 2 * PW - 2].abs() + 10.0
    if PH > 1:
        x[0, 3, 0] = x[0, 3, 1] = x[0, 2, 0].abs() + 10.0
    x[B - 1, 1, 0, 0] = float("nan")
    dy = rnd(B * PH * PW, C, seed=92)
    xr = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    y, idx = F.max_pool2d(xr, 2, 2, return_indices=True)
    y.backward(dy.double().view(B, PH, PW, C).permute(0, 3, 1, 2))
    taps = 2 * ((idx // W) % 2) + (idx % W) % 2
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C)  # noqa: E731
    return x.reshape(-1, C), dy, rows(y.detach()), rows(taps), rows(xr.grad)


@gpu
@pytest.mark.parametrize("B,H,W,C", POOLS)
def test_maxpool2_against_torch(L, B, H, W, C):
    x, dy, y_ref, taps_ref, dx_ref = pool_case(B, H, W, C)
    PH, PW = H // 2, W // 2
    xp = Poisoned(x, ld=C + 3)
    y, arg = Guarded(B * PH * PW, C), Guarded(B * PH * PW, C, dtype=torch.uint8)
    assert L.vc_maxpool2_fwd(B, H, W, C, xp.ptr, C + 3, y.ptr, arg.ptr, S()) == 0
    got, taps = y.check(), arg.check()
    assert torch.equal(torch.isnan(got), torch.isnan(y_ref)) and int(torch.isnan(got).sum()) == 1
    assert torch.equal(got.nan_to_num(7.0).double(), y_ref.nan_to_num(7.0))
    assert torch.equal(taps.long(), taps_ref)
    c = C - 1       # (channel 0 of a one-element batch holds the NaN)
    assert int(taps[0, c]) == 0 and (PW == 1 or int(taps[PW - 1, c]) == 1) and (PH == 1 or int(taps[PW, c]) == 2)
    dyp = Poisoned(dy)
    dx = Guarded(B * H * W, C, ld=C + 5)
    assert L.vc_maxpool2_bwd(B, H, W, C, dyp.ptr, arg.ptr, dx.ptr, C + 5, S()) == 0
    gdx = dx.check()
    assert torch.equal(gdx.double(), dx_ref)
    g4 = gdx.view(B, H, W, C)
    if H % 2:
        assert not g4[:, H - 1].any()
    if W % 2:
        assert not g4[:, :, W - 1].any()


# ------------------------------------------------------------------------------------------ conv.hip: im2col / col2im
COLS = [(2, 5, 9, 70), (3, 9, 5, 64), (1, 3, 7, 4)]


def unfold_rows(x64, B, H, W, C):
    """[B H W, C] float64 -> the col matrix [B OH OW, 9 C], k = c * 9 + kh * 3 + kw"""
    return F.unfold(x64.view(B, H, W, C).permute(0, 3, 1, 2), 3).permute(0, 2, 1).reshape(-1, 9 * C)


def fold_rows(dcol64, B, H, W, C):
    d = F.fold(dcol64.view(B, (H - 2) * (W - 2), 9 * C).permute(0, 2, 1), (H, W), 3)
    return d.permute(0, 2, 3, 1).reshape(-1, C)


def im2col_col2im(lib, B, H, W, C, with_bn):
    x, dcol = rnd(B * H * W, C, seed=71), rnd(B * (H - 2) * (W - 2), 9 * C, seed=76)
    bn = (rnd(C, seed=72), rnd(C, seed=73).abs() + 0.5, rnd(C, seed=74), rnd(C, seed=75))
    keep, bp = bn_ptrs(bn, with_bn)
    xp, dp = Poisoned(x), Poisoned(dcol)
    col, dx = Guarded(B * (H - 2) * (W - 2), 9 * C), Guarded(B * H * W, C)
    assert lib.vc_im2col3x3(B, H, W, C, xp.ptr, *bp, col.ptr, S()) == 0
    assert lib.vc_col2im3x3(B, H, W, C, dp.ptr, dx.ptr, S()) == 0
    x64 = x.double()
    if with_bn:
        mean, inv, g, b = (t.double() for t in bn)
        x64 = (x64 - mean) * (inv * g) + b
    return col.check(), unfold_rows(x64, B, H, W, C), dx.check(), fold_rows(dcol.double(), B, H, W, C)


@gpu
@pytest.mark.parametrize("with_bn", [False, True])
@pytest.mark.parametrize("B,H,W,C", COLS)
def test_im2col_col2im_rectangular(L, B, H, W, C, with_bn):
    col, col_ref, dx, dx_ref = im2col_col2im(L, B, H, W, C, with_bn)
    shape = f"B={B},H={H},W={W},C={C},bn={int(with_bn)}"
    if with_bn:
        within("im2col3x3 (affine)", shape, rel_err(col.numpy(), col_ref.numpy()), 1e-5)
    else:
        assert torch.equal(col.double(), col_ref)
    within("col2im3x3", shape, rel_err(dx.numpy(), dx_ref.numpy()), 1e-5)


@gpu
@pytest.mark.parametrize("B,H,W,C", COLS)
def test_im2col_col2im_rectangular_lds_forms(B, H, W, C, monkeypatch):
    """the LDS-staged and the per-thread forms (probe library, VITCNN_C2I_LDS) bit for bit, both guarded"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vitcnn_amd._lib import probe_lib
    outs = []
    for lds in ("1", "0"):
        monkeypatch.setenv("VITCNN_C2I_LDS", lds)
        outs.append(im2col_col2im(probe_lib(), B, H, W, C, True))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][2], outs[1][2])
    within("im2col3x3 (affine, per-thread form)", f"B={B},H={H},W={W},C={C}",
           rel_err(outs[1][0].numpy(), outs[1][1].numpy()), 1e-5)
    within("col2im3x3 (per-thread form)", f"B={B},H={H},W={W},C={C}", rel_err(outs[1][2].numpy(), outs[1][3].numpy()), 1e-5)


@gpu
@pytest.mark.parametrize("B,H,W,C", COLS)
def test_bn_im2col_rectangular(L, big, B, H, W, C):
    """train-mode BatchNorm over the B H W rows + im2col of the normalised map, against float64 batch_norm + unfold"""
    x = rnd(B * H * W, C, seed=81, scale=2.0) + 3.0
    w, b = rnd(C, seed=82) + 1.5, rnd(C, seed=83)
    rm0, rv0 = rnd(C, seed=84), rnd(C, seed=85).abs() + 0.5
    xp, wd, bd = Poisoned(x), w.to(DEV), b.to(DEV)
    sm, si, rm, rv = Guarded(1, C), Guarded(1, C), Guarded(1, C, init=rm0), Guarded(1, C, init=rv0)
    col = Guarded(B * (H - 2) * (W - 2), 9 * C)
    assert L.vc_bn_im2col3x3(B, H, W, C, xp.ptr, 1e-5, 0.1, sm.ptr, si.ptr, rm.ptr, rv.ptr, P(wd), P(bd), col.ptr,
                             P(big), big.numel(), S()) == 0
    x64, rm64, rv64 = x.double(), rm0.double(), rv0.double()
    y64 = F.batch_norm(x64, rm64, rv64, w.double(), b.double(), True, 0.1, 1e-5)
    shape = f"B={B},H={H},W={W},C={C}"
    within("bn_im2col3x3 col", shape, rel_err(col.check().numpy(), unfold_rows(y64, B, H, W, C).numpy()), 1e-5)
    within("bn_im2col3x3 mean", shape, rel_err(sm.check()[0].numpy(), x64.mean(0).numpy()), 1e-5)
    within("bn_im2col3x3 invstd", shape,
           rel_err(si.check()[0].numpy(), torch.rsqrt(x64.var(0, unbiased=False) + 1e-5).numpy()), 1e-5)
    within("bn_im2col3x3 running_mean", shape, rel_err(rm.check()[0].numpy(), rm64.numpy()), 1e-5)
    within("bn_im2col3x3 running_var", shape, rel_err(rv.check()[0].numpy(), rv64.numpy()), 1e-5)

