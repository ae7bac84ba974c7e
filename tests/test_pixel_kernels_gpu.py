"""Per-kernel parity of csrc/pixel.hip on the MI355X against float64 written here from the formulas in
include/vitcnn.h: the fused fully-connected layer (Linear + BatchNorm1d + ReLU / sigmoid / plain) forward and
backward, EndNet's loss, SpectralFormer's embedding forward and backward.

Shapes are the smallest at which the kernels can go wrong: K from 1 (the LiDAR band) over odd sizes to 256, N = 12
(one and a half column groups of 8), 16 and 128, B = 2 and 3 (fewer rows than row groups), 64, 65 and the train bound
1024; ldx = K (unaligned rows) and a padded ldx with NaN in the gap; ldy > N writing the second half of a wider
buffer.  Outputs start as NaN and are followed by a guard region (helpers.Guarded) that must stay untouched; padded
inputs carry NaN in their gap columns (helpers.Poisoned).  A second call repeats its bits.

Inputs: x ~ U(-1, 1); W with |w| in [0.5, 1.5] / sqrt(K) and random signs, so that no column's batch variance
degenerates (at K = 1 a column is x w + b: with |w| -> 0 its BatchNorm would divide fp32 rounding by ~0 in any
implementation); the seed advances until every float64 BatchNorm output is >= 1e-5 away from 0 (no ReLU decision
hangs on rounding; nothing is excluded).

Tolerances: 1e-5 of the reference's largest |value| for every output, forward and backward
(test_mdlrs_kernels_gpu.py's bound).  Only where a BatchNorm case misses it, the existing path is measured on the same
inputs against the same float64 -- forward: vc_gemm_colstats + vc_bn_apply_partials; backward: vc_bn_bwd_relu_ex + the
weight-gradient vc_gemm_ex with the bias gradient riding on it -- and at most twice its error is allowed; both figures
are printed.  (At B = 2 or 3 a train-mode BatchNorm's dz is a difference of terms up to ~1e5 times larger than itself
in exact arithmetic, which no fp32 evaluation resolves to 1e-5 of the result.)
"""
import functools

import pytest
import torch

from helpers import Guarded, Poisoned, within

pytestmark = pytest.mark.gpu
DEV = "cuda"
PLAIN, BN_RELU, SIGMOID = 0, 1, 2
BMAX = 1024
EPS, MOM = 1e-5, 0.1


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vitcnn_amd._lib import lib
    return lib()


def S():
    return torch.cuda.current_stream().cuda_stream


def uni(g, *shape, lo=-1.0, hi=1.0):
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()


def fc_ref(mode, train, x, W, b, gamma, beta, rm, rv):
    """float64 forward from the header's formulas"""
    x, W, b = x.double(), W.double(), b.double()
    B = x.shape[0]
    z = x @ W.t() + b
    r = dict(z=z)
    if mode == PLAIN:
        r["y"] = z
    elif mode == SIGMOID:
        r["y"] = 1.0 / (1.0 + torch.exp(-z))
    else:
        if train:
            mean, var = z.mean(0), z.var(0, unbiased=False)
            r["rm"] = (1 - MOM) * rm.double() + MOM * mean
            r["rv"] = (1 - MOM) * rv.double() + MOM * var * B / (B - 1)
        else:
            mean, var = rm.double(), rv.double()
        rstd = 1.0 / torch.sqrt(var + EPS)
        xhat = (z - mean) * rstd
        pre = xhat * gamma.double() + beta.double()
        r.update(mean=mean, rstd=rstd, xhat=xhat, pre=pre, y=torch.relu(pre))
    return r


def fc_bwd_ref(mode, train, r, x, dy, gamma):
    """float64 backward from the header's formulas"""
    x, dy = x.double(), dy.double()
    B = x.shape[0]
    out = {}
    if mode == PLAIN:
        dz = dy
    elif mode == SIGMOID:
        dz = dy * r["y"] * (1 - r["y"])
    else:
        g = dy * (r["y"] > 0)
        dbeta, dgamma = g.sum(0), (g * r["xhat"]).sum(0)
        sc = gamma.double() * r["rstd"]
        dz = sc * (g - dbeta / B - r["xhat"] * dgamma / B) if train else sc * g
        out.update(dbeta=dbeta, dgamma=dgamma)
    out.update(dz=dz, dW=dz.t() @ x, db=dz.sum(0))
    return out


@functools.lru_cache(maxsize=None)
def fc_case(mode, train, B, K, N):
    """seeded inputs of one layer and its float64 reference; the seed advances until every BatchNorm output keeps
    1e-5 from 0"""
    for seed in range(1, 200):
        g = torch.Generator().manual_seed(1000 * seed + 7 * B + 3 * K + N)
        x = uni(g, B, K)
        W = uni(g, N, K, lo=0.5, hi=1.5) * (torch.randint(0, 2, (N, K), generator=g) * 2 - 1).float() / K ** 0.5
        b = uni(g, N)
        gamma, beta = uni(g, N, lo=0.5, hi=1.5), uni(g, N, lo=-0.5, hi=0.5)
        rm, rv = uni(g, N, lo=-0.3, hi=0.3), uni(g, N, lo=0.5, hi=1.5)
        dy = uni(g, B, N)
        ref = fc_ref(mode, train, x, W, b, gamma, beta, rm, rv)
        if mode != BN_RELU or float(ref["pre"].abs().min()) >= 1e-5:
            return dict(x=x, W=W, b=b, gamma=gamma, beta=beta, rm=rm, rv=rv, dy=dy, ref=ref, seed=seed)
    raise AssertionError("no seed keeps the BatchNorm outputs away from 0")


def err(got, ref):
    return float((got.double() - ref).abs().max())


def run_fc_fwd(L, c, mode, train, B, K, N, ldx, ldy, col0):
    """one forward into columns col0 .. col0 + N - 1 of a [B, ldy] buffer; returns y, xhat, mean, rstd, rm, rv (CPU)"""
    d = lambda t: t.to(DEV).contiguous()
    xin = Poisoned(c["x"], ld=ldx)
    W, b = d(c["W"]), d(c["b"])
    bn = mode == BN_RELU
    gamma, beta, rm, rv = (d(c[k]) for k in ("gamma", "beta", "rm", "rv"))
    wide = Guarded(B, ldy)                 # the whole [B, ldy] buffer: NaN outside the written columns must survive
    y_ptr = wide.ptr + 4 * col0
    xhat, sm, sr = Guarded(B, N), Guarded(1, N), Guarded(1, N)
    L.vc_fc_fused_fwd(mode, train, B, K, N, xin.ptr, ldx, W.data_ptr(), b.data_ptr(),
                      gamma.data_ptr() if bn else None, beta.data_ptr() if bn else None,
                      rm.data_ptr() if bn else None, rv.data_ptr() if bn else None, EPS, MOM, y_ptr, ldy,
                      xhat.ptr if bn else None, sm.ptr if bn else None, sr.ptr if bn else None, S())
    full = wide.check()
    y = full[:, col0:col0 + N]
    other = torch.cat([full[:, :col0], full[:, col0 + N:]], 1)
    assert bool(torch.isnan(other).all()), "store outside the layer's columns of the wider buffer"
    if bn:
        return y, xhat.check(), sm.check()[0], sr.check()[0], rm.cpu(), rv.cpu()
    xhat.check(), sm.check(), sr.check()
    return y, None, None, None, None, None


def two_launch_bn(L, c, B, K, N):
    """the existing two-launch Linear + train-mode BatchNorm + ReLU (vc_gemm_colstats + vc_bn_apply_partials) on the
    same inputs: y, xhat (= (C - mean) * invstd of its own outputs), mean, rstd, running statistics.  It wants K a
    multiple of 4: zero columns pad x and W (they add exact zeros to every product)."""
    K4 = (K + 3) // 4 * 4
    x, W = torch.zeros(B, K4), torch.zeros(N, K4)
    x[:, :K], W[:, :K] = c["x"], c["W"]
    d = lambda t: t.to(DEV).contiguous()
    x, W, b, gamma, beta, rm, rv = (d(t) for t in (x, W, c["b"], c["gamma"], c["beta"], c["rm"], c["rv"]))
    P_ = -(-B // 64)
    pre, y = torch.empty(B, N, device=DEV), torch.empty(B, N, device=DEV)
    cs = torch.empty(P_ * 2 * N, dtype=torch.float64, device=DEV)
    mean, inv = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    L.vc_gemm_colstats(B, N, K4, x.data_ptr(), K4, W.data_ptr(), K4, b.data_ptr(), pre.data_ptr(), N, 0, cs.data_ptr(), S())
    L.vc_bn_apply_partials(B, N, pre.data_ptr(), N, P_, cs.data_ptr(), b.data_ptr(), EPS, MOM, mean.data_ptr(),
                           inv.data_ptr(), rm.data_ptr(), rv.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1,
                           y.data_ptr(), N, S())
    torch.cuda.synchronize()
    return dict(y=y.cpu(), xhat=((pre - mean) * inv).cpu(), mean=mean.cpu(), rstd=inv.cpu(), rm=rm.cpu(), rv=rv.cpu())


def check_fc_fwd(tag, shape, got, c, mode, train, fallback=None):
    """every output within 1e-5 of the reference's largest |value|.  `fallback` (train-mode BatchNorm only; a function
    returning two_launch_bn's outputs) is consulted only where that bound is missed: the existing two-launch path's
    error on the same inputs against the same float64 is measured, and at most twice that error is allowed (a column
    whose batch variance is comparable to eps -- two rows that nearly agree -- amplifies the fp32 rounding of x W^T
    in any implementation).  Both figures are printed."""
    ref = c["ref"]
    y, xhat, mean, rstd, rm, rv = got
    scale = lambda t: max(float(t.abs().max()), 1e-30)
    cache = {}

    def hold(name, value, key):
        e, bound = err(value, ref[key]), 1e-5 * scale(ref[key])
        if e >= bound and fallback is not None:
            if not cache:
                cache.update(fallback())
            e2 = err(cache[name], ref[key])
            print(f"PARITY two_launch.{tag}.{name} {shape} {e2:.3e} (the existing path; the fused layer may reach twice it)")
            bound = max(bound, 2 * e2)
        within(f"fc_fwd.{tag}.{name}", shape, e, bound, inclusive=e >= 1e-5 * scale(ref[key]))

    hold("y", y, "y")
    if mode == BN_RELU:
        hold("xhat", xhat, "xhat")
        hold("mean", mean, "mean")
        hold("rstd", rstd, "rstd")
        assert bool(((y > 0) == (ref["y"] > 0)).all())
        if train:
            hold("rm", rm, "rm")
            hold("rv", rv, "rv")
        else:
            assert torch.equal(rm, c["rm"]) and torch.equal(rv, c["rv"])     # eval leaves them alone


def run_fc_bwd(L, c, mode, train, B, K, N, ldx, lddy, with_dz=True):
    """the backward fed with the float64 forward's values rounded to fp32 (so it is judged on its own)"""
    ref = c["ref"]
    d = lambda t: t.float().to(DEV).contiguous()
    bn = mode == BN_RELU
    xin, dyin = Poisoned(c["x"], ld=ldx), Poisoned(c["dy"], ld=lddy)
    yin = Poisoned(ref["y"].float(), ld=N + 5)
    xhat = d(ref["xhat"]) if bn else None
    gamma = d(c["gamma"]) if bn else None
    rstd = d(ref["rstd"]) if bn else None
    dz, dW, db = Guarded(B, N, ld=N + 3), Guarded(N, K), Guarded(1, N)
    dga, dbe = Guarded(1, N), Guarded(1, N)
    L.vc_fc_fused_bwd(mode, train, B, K, N, dyin.ptr, lddy, yin.ptr if mode != PLAIN else None, N + 5,
                      xhat.data_ptr() if bn else None, xin.ptr, ldx, gamma.data_ptr() if bn else None,
                      rstd.data_ptr() if bn else None, dz.ptr if with_dz else None, N + 3, dW.ptr, db.ptr,
                      dga.ptr if bn else None, dbe.ptr if bn else None, S())
    out = dict(dz=dz.check(), dW=dW.check(), db=db.check()[0], dgamma=dga.check()[0], dbeta=dbe.check()[0])
    if not with_dz:
        assert bool(torch.isnan(out["dz"]).all())
    return out


def existing_bn_bwd(L, c, train, B, K, N):
    """the existing backward of Linear + BatchNorm + ReLU on the same inputs: vc_bn_bwd_relu_ex (fed the float64
    pre-norm z, mean and rstd rounded to fp32; it recomputes the ReLU decisions from them) for dz, dgamma, dbeta, then
    the weight-gradient vc_gemm_ex with the bias gradient in its epilogue for dW, db"""
    from vitcnn_amd.model import N_COUNTERS
    from vitcnn_amd.program import counters
    ref = c["ref"]
    d = lambda t: t.float().to(DEV).contiguous()
    x, dy, z, mean, rstd, gamma, beta = (d(t) for t in (c["x"], c["dy"], ref["z"], ref["mean"], ref["rstd"], c["gamma"],
                                                        c["beta"]))
    nws = 1 << 22
    ws = torch.empty(nws, device=DEV)
    cnt = counters(torch.device(DEV, torch.cuda.current_device()), S())
    dz, dga, dbe = torch.empty(B, N, device=DEV), torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    dW, db = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
    L.vc_bn_bwd_relu_ex(train, B, N, dy.data_ptr(), N, z.data_ptr(), N, mean.data_ptr(), rstd.data_ptr(),
                        gamma.data_ptr(), beta.data_ptr(), dz.data_ptr(), N, 0.0, dga.data_ptr(), dbe.data_ptr(), 0.0,
                        ws.data_ptr(), nws, cnt, N_COUNTERS, S())
    L.vc_gemm_ex(1, 0, N, K, B, 1.0, dz.data_ptr(), N, 0, x.data_ptr(), K, 0, 0.0, dW.data_ptr(), K, 0, 1, None, None, 0,
                 0, 0, db.data_ptr(), ws.data_ptr(), nws, cnt, N_COUNTERS, S())
    torch.cuda.synchronize()
    return dict(dz=dz.cpu(), dW=dW.cpu(), db=db.cpu(), dgamma=dga.cpu(), dbeta=dbe.cpu())


def check_fc_bwd(tag, shape, got, c, mode, train, fallback=None):
    """every output within 1e-5 of the reference's largest |value|; `fallback` (BatchNorm modes; a function returning
    existing_bn_bwd's outputs) is consulted only where that is missed: at most twice the existing path's error on the
    same inputs against the same float64 is allowed, and both figures are printed"""
    want = fc_bwd_ref(mode, train, c["ref"], c["x"], c["dy"], c["gamma"])
    cache = {}
    for k in ("dz", "dW", "db") + (("dgamma", "dbeta") if mode == BN_RELU else ()):
        e, base = err(got[k], want[k]), 1e-5 * max(float(want[k].abs().max()), 1e-30)
        bound = base
        if e >= base and fallback is not None:
            if not cache:
                cache.update(fallback())
            e2 = err(cache[k], want[k])
            print(f"PARITY existing.{tag}.{k} {shape} {e2:.3e} vs 1e-5 of the largest value {base:.3e} "
                  f"(the existing path; the fused layer may reach twice it)")
            bound = max(base, 2 * e2)
        within(f"fc_bwd.{tag}.{k}", shape, e, bound, inclusive=e >= base)


FC_K = [1, 2, 13, 63, 144, 256]
FC_N = [12, 16, 128]
FC_B = [2, 3, 64, 65, BMAX]


@pytest.mark.parametrize("B", FC_B)
@pytest.mark.parametrize("N", FC_N)
@pytest.mark.parametrize("K", FC_K)
def test_fc_fused_batchnorm_relu_train(L, K, N, B):
    """Linear + BatchNorm1d (batch statistics, running-statistics update) + ReLU in one launch and its backward, with
    ldx = K into the second half of a [B, 2 N + 3] buffer and with a padded ldx into the first; each twice: same bits"""
    c = fc_case(BN_RELU, 1, B, K, N)
    shape = f"B{B} K{K} N{N}"
    for ldx, ldy, col0 in ((K, 2 * N + 3, N + 3), (K + 3, N + 1, 0)):
        got = run_fc_fwd(L, c, BN_RELU, 1, B, K, N, ldx, ldy, col0)
        check_fc_fwd("bn_train", shape + f" ldx{ldx}", got, c, BN_RELU, 1, fallback=lambda: two_launch_bn(L, c, B, K, N))
        again = run_fc_fwd(L, c, BN_RELU, 1, B, K, N, ldx, ldy, col0)
        assert all(torch.equal(a, b) for a, b in zip(got, again))
        bw = run_fc_bwd(L, c, BN_RELU, 1, B, K, N, ldx, 2 * N if col0 else N)
        check_fc_bwd("bn_train", shape + f" ldx{ldx}", bw, c, BN_RELU, 1,
                     fallback=lambda: existing_bn_bwd(L, c, 1, B, K, N))
        again = run_fc_bwd(L, c, BN_RELU, 1, B, K, N, ldx, 2 * N if col0 else N)
        assert all(torch.equal(bw[k], again[k]) for k in bw)


@pytest.mark.parametrize("mode,train", [(BN_RELU, 0), (SIGMOID, 0), (PLAIN, 0)], ids=["bn_eval", "sigmoid", "plain"])
@pytest.mark.parametrize("B", [1, 3, 65, 300, 1100])
@pytest.mark.parametrize("K,N", [(1, 12), (13, 16), (144, 128), (256, 12), (16, 145)])
def test_fc_fused_row_tiled_modes(L, K, N, B, mode, train):
    """eval-mode BatchNorm (running statistics), sigmoid and plain on the row-tiled grid: any B (1, within one 128-row
    tile, across three, above the train bound); the backward up to its bound, with and without dz"""
    c = fc_case(mode, train, B, K, N)
    name = {BN_RELU: "bn_eval", SIGMOID: "sigmoid", PLAIN: "plain"}[mode]
    shape = f"B{B} K{K} N{N}"
    for ldx, ldy, col0 in ((K, 2 * N + 3, N + 3), (K + 3, N, 0)):
        got = run_fc_fwd(L, c, mode, train, B, K, N, ldx, ldy, col0)
        check_fc_fwd(name, shape + f" ldx{ldx}", got, c, mode, train)
        again = run_fc_fwd(L, c, mode, train, B, K, N, ldx, ldy, col0)
        assert torch.equal(got[0], again[0])
        if B <= BMAX:
            bw = run_fc_bwd(L, c, mode, train, B, K, N, ldx, N + 2, with_dz=col0 == 0)
            if col0:
                bw["dz"] = fc_bwd_ref(mode, train, c["ref"], c["x"], c["dy"], c["gamma"])["dz"]   # not written: skip
            check_fc_bwd(name, shape + f" ldx{ldx}", bw, c, mode, train,
                         fallback=(lambda: existing_bn_bwd(L, c, 0, B, K, N)) if mode == BN_RELU else None)


def test_fc_fused_refuses_what_it_cannot_hold(L):
    """train-mode BatchNorm above the LDS bound is an error code, never another computation; eval takes the same B"""
    c = fc_case(BN_RELU, 0, 1100, 13, 16)
    d = lambda t: t.to(DEV).contiguous()
    x, W, b, gamma, beta, rm, rv = (d(c[k]) for k in ("x", "W", "b", "gamma", "beta", "rm", "rv"))
    y, xhat, st = Guarded(1100, 16), Guarded(1100, 16), Guarded(2, 16)
    args = lambda train, B: (BN_RELU, train, B, 13, 16, x.data_ptr(), 13, W.data_ptr(), b.data_ptr(), gamma.data_ptr(),
                             beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), EPS, MOM, y.ptr, 16, xhat.ptr, st.ptr,
                             st.ptr + 64, S())
    assert L.raw["vc_fc_fused_fwd"](*args(1, BMAX + 1)) == 1
    assert L.raw["vc_fc_fused_fwd"](*args(1, 1)) == 1
    assert bool(torch.isnan(y.check()).all()) and torch.equal(rm.cpu(), c["rm"])
    assert L.raw["vc_fc_fused_fwd"](*args(0, 1100)) == 0
    assert torch.isfinite(y.check()).all()


# ---------------------------------------------------------------------------------------------- EndNet loss
LOSS_SHAPES = [(1, 12, 5, 1), (3, 16, 13, 2), (64, 16, 144, 1), (70, 12, 30, 1)]


def loss_inputs(B, ncls, C1, C2):
    g = torch.Generator().manual_seed(B * 100 + ncls)
    out = uni(g, B, ncls, lo=-3, hi=3)
    t = torch.randint(0, ncls, (B,), generator=g)
    if B > 1:
        t[0] = 0                     # a sample of the zero-weight class
    t[-1] = 1
    w = uni(g, ncls, lo=0.5, hi=2.0)
    w[0] = 0.0
    return out, t, w, uni(g, B, C1, lo=0, hi=1), uni(g, B, C1, lo=0, hi=1), uni(g, B, C2, lo=0, hi=1), \
        uni(g, B, C2, lo=0, hi=1)


def run_loss(L, out, t, w, de1, x1, de2, x2):
    B, ncls = out.shape
    C1, C2 = de1.shape[1], de2.shape[1]
    d = lambda a: a.to(DEV).contiguous()
    o, tt, ww, a1, b1, a2, b2 = (d(a) for a in (out, t, w, de1, x1, de2, x2))
    loss, dout, d1, d2 = Guarded(1, 1), Guarded(B, ncls), Guarded(B, C1), Guarded(B, C2)
    L.vc_endnet_loss_fwd_bwd(B, ncls, C1, C2, o.data_ptr(), tt.data_ptr(), ww.data_ptr(), a1.data_ptr(), b1.data_ptr(),
                             a2.data_ptr(), b2.data_ptr(), loss.ptr, dout.ptr, d1.ptr, d2.ptr, S())
    return loss.check()[0, 0], dout.check(), d1.check(), d2.check()


@pytest.mark.parametrize("B,ncls,C1,C2", LOSS_SHAPES)
def test_endnet_loss_against_float64(L, B, ncls, C1, C2):
    out, t, w, de1, x1, de2, x2 = loss_inputs(B, ncls, C1, C2)
    o64 = out.double().requires_grad_(True)
    a1, a2 = de1.double().requires_grad_(True), de2.double().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(o64, t, weight=w.double()) + ((a1 - x1.double()) ** 2).mean() + \
        ((a2 - x2.double()) ** 2).mean()
    ref.backward()
    got = run_loss(L, out, t, w, de1, x1, de2, x2)
    shape = f"B{B} ncls{ncls} C{C1}+{C2}"
    within("endnet_loss.loss", shape, abs(float(got[0]) - float(ref.detach())), 1e-5 * abs(float(ref.detach())))
    for name, g, r in (("dout", got[1], o64.grad), ("dde1", got[2], a1.grad), ("dde2", got[3], a2.grad)):
        within("endnet_loss." + name, shape, err(g, r), 1e-5 * float(r.abs().max()))
    assert not got[1][t == 0].any()          # the zero-weight class's samples get no gradient
    again = run_loss(L, out, t, w, de1, x1, de2, x2)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("B,ncls,C1,C2", LOSS_SHAPES)
def test_endnet_loss_with_exact_reconstruction_is_the_cross_entropy_kernel_bit_for_bit(L, B, ncls, C1, C2):
    out, t, w, _, x1, _, x2 = loss_inputs(B, ncls, C1, C2)
    got = run_loss(L, out, t, w, x1, x1, x2, x2)
    o, tt, ww = out.to(DEV), t.to(DEV), w.to(DEV)
    loss, dout = Guarded(1, 1), Guarded(B, ncls)
    L.vc_ce_fwd_bwd(B, ncls, o.data_ptr(), tt.data_ptr(), ww.data_ptr(), -100, loss.ptr, dout.ptr, S())
    assert torch.equal(got[0], loss.check()[0, 0]) and torch.equal(got[1], dout.check())
    assert not got[2].any() and not got[3].any()


# ---------------------------------------------------------------------------------------------- SpectralFormer embedding
EMB_BANDS = [(1, 0), (13, 2), (144, 1), (254, 1)]      # T = 2, 16, 146, 256


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("C1,C2", EMB_BANDS)
def test_sf_embed_forward_and_backward(L, C1, C2, B, p):
    D = 64 if C1 != 13 else 20
    T = C1 + C2 + 1
    g = torch.Generator().manual_seed(T * 10 + B)
    x1, x2 = uni(g, B, C1, lo=0, hi=1), uni(g, B, max(C2, 1), lo=0, hi=1)
    w, bias, cls, pos, dX = uni(g, D), uni(g, D), uni(g, D), uni(g, T, D), uni(g, B, T, D)
    seed = 0x1234567 + T
    d = lambda a: a.to(DEV).contiguous()
    a1, a2, dw_, db_, dc_, dp_ = (d(a) for a in (x1, x2, w, bias, cls, pos))
    n = B * T * D

    def fwd():
        X, mask = Guarded(B * T, D), Guarded(1, n, dtype=torch.uint8)
        L.vc_sf_embed_fwd(B, C1, C2, D, a1.data_ptr(), a2.data_ptr() if C2 else None, dw_.data_ptr(), db_.data_ptr(),
                          dc_.data_ptr(), dp_.data_ptr(), p, seed, X.ptr, mask.ptr if p > 0 else None, S())
        return X.check().view(B, T, D), mask.check()[0]

    X, mask = fwd()
    shape = f"B{B} T{T} D{D} p{p}"
    x = torch.cat([x1, x2[:, :C2]], 1).double()
    ref = torch.cat([(cls.double() + pos[0].double()).expand(B, 1, D),
                     x.unsqueeze(-1) * w.double() + bias.double() + pos[1:].double()], 1)
    keep = torch.ones(B, T, D, dtype=torch.float64)
    if p > 0:
        # the mask is vc_dropout_fwd's for the same seed over the same element index
        src = torch.zeros(n, device=DEV)
        y, mk = Guarded(1, n), Guarded(1, n, dtype=torch.uint8)
        L.vc_dropout_fwd(n, src.data_ptr(), None, y.ptr, mk.ptr, p, seed, S())
        assert torch.equal(mask, mk.check()[0])
        keep = mask.view(B, T, D).double()
        if n > 1000:
            assert abs(float(keep.mean()) - (1 - p)) < 0.05
        ref = ref * keep / (1 - p)
    else:
        assert bool((mask == 0xA5).all())        # no mask is written without dropout
    within("sf_embed_fwd", shape, err(X, ref), 1e-5 * float(ref.abs().max()))
    X2, mask2 = fwd()
    assert torch.equal(X, X2) and torch.equal(mask, mask2)

    def bwd():
        gdw, gdb, gdp, gdc = Guarded(1, D), Guarded(1, D), Guarded(T, D), Guarded(1, D)
        ws = torch.empty(T * D, device=DEV)
        dXd, md = d(dX), d(mask)
        L.vc_sf_embed_bwd(B, C1, C2, D, a1.data_ptr(), a2.data_ptr() if C2 else None, dXd.data_ptr(),
                          md.data_ptr() if p > 0 else None, p, gdw.ptr, gdb.ptr, gdp.ptr, gdc.ptr, ws.data_ptr(), T * D, S())
        return gdw.check()[0], gdb.check()[0], gdp.check(), gdc.check()[0]

    got = bwd()
    gX = dX.double() * keep / (1 - p)
    want = ((x.unsqueeze(-1) * gX[:, 1:]).sum((0, 1)), gX[:, 1:].sum((0, 1)), gX.sum(0), gX[:, 0].sum(0))
    for name, a, r in zip(("dw", "db", "dpos", "dcls"), got, want):
        within("sf_embed_bwd." + name, shape, err(a, r), 1e-5 * max(float(r.abs().max()), 1e-30))
    assert all(torch.equal(a, b) for a, b in zip(got, bwd()))
