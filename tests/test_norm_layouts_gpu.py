"""LayerNorm and BatchNorm (csrc/norm.hip) off their natural layouts, on the MI355X, against float64 torch on the
CPU over the fp32 inputs widened: every leading dimension above C and distinct (inputs helpers.Poisoned: gap
columns NaN; outputs helpers.Guarded), C on both sides of the 64-lane row and of the 64-channel block, one row and
one channel, null dw / db, dw and db apart (off the `db == dw + C` fast path), partial workspaces exactly as large
as the plan needs (guarded) and so small that ln_partial_rows doubles, the split LayerNorm backward, BatchNorm in
train and eval mode with the unbiased running variance at M = 2, through a ReLU read from the forward's output or
recomputed from the affine, and without dx.

Bounds: 1e-5 of max |ref| forward, 1e-4 for the gradients.  Rows / channels of mean 1000 with unit spread tell a
two-pass variance from E[x^2] - mean^2; there the reference implementation's own fp32 error sets the scale: the
kernel's max deviation from float64 must stay within 4 x (torch fp32 CPU's deviation on the same input) +
2 eps32 max |ref| (mean1000_rule_*: the rule is far below a one-pass variance's error, checked without a GPU).
"""
import pytest
import torch

from helpers import EPS32, Guarded, Poisoned, rel_err, within

gpu = pytest.mark.gpu
DEV = "cuda"
F = torch.nn.functional
LN_EPS, BN_EPS, MOM = 1e-6, 1e-5, 0.1


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vitcnn_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def ws():
    return torch.empty(1 << 20, device=DEV)


@pytest.fixture(scope="module")
def cnt():
    return torch.zeros(1 << 10, dtype=torch.int32, device=DEV)


def S():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return t.data_ptr() if t is not None else None


def uni(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * (0.97130763 * scale)


def max_dev(a, b):
    return float((a.double() - b.double()).abs().max())


def rule(ref, torch32):
    """section 16's GELU rule: 4 x the fp32 reference implementation's deviation + 2 eps32 max |ref|"""
    return 4.0 * max_dev(torch32, ref) + 2.0 * EPS32 * float(ref.abs().max())


def regime_input(regime, rows, C, seed):
    """uniform: U(-3, 3) + 0.5.  const: the same with the first and the last row constant 0.75 (every fp32 partial
    sum of up to 512 copies of 0.75 is exact, so the fp32 mean is 0.75, the variance 0 and y = b: with
    rstd = eps^-1/2 = 1000 a one-ulp mean error would be amplified a thousandfold in any fp32 LayerNorm).
    mean1000: 1000 + unit spread, per row and per channel."""
    x = uni(rows, C, seed=seed, scale=3.0) + 0.5
    if regime == "const":
        x[0] = 0.75
        x[rows - 1] = 0.75
    elif regime == "mean1000":
        x = (1000.0 + uni(rows, C, seed=seed, scale=3.0 ** 0.5)).float()
    return x


def check(name, shape, got, ref, bound, regime, torch32=None):
    """the fixed relative bound, or in the mean-1000 regime the 4 x torch fp32 + 2 eps32 rule on the max deviation"""
    if regime == "mean1000" and torch32 is not None:
        within(name + " (mean 1000: max abs dev)", shape, max_dev(got, ref), rule(ref, torch32), inclusive=True)
    else:
        within(name, shape, rel_err(got.numpy(), ref.numpy()), bound)


# ------------------------------------------------------------------------------------------ the rule, on the CPU
def one_pass_layer_norm32(x, w, b, eps):
    mean = x.mean(1, keepdim=True)
    var = (x * x).mean(1, keepdim=True) - mean * mean
    return (x - mean) * torch.rsqrt(var.clamp_min(0) + eps) * w + b


def test_mean1000_rule_separates_one_pass_layernorm():
    """no GPU: on rows of mean 1000 and unit spread torch's fp32 layer_norm stays far from the one-pass failure
    level eps32 mean^2 / var ~ 0.06, so the rule's bound lies well below it, and an fp32 E[x^2] - mean^2 LayerNorm
    written here misses that bound"""
    for R, C in [(9, 63), (100, 64), (5, 512)]:
        x, w, b = regime_input("mean1000", R, C, 1), uni(C, seed=2) + 1.5, uni(C, seed=3)
        ref = F.layer_norm(x.double(), (C,), w.double(), b.double(), LN_EPS)
        t32 = F.layer_norm(x, (C,), w, b, LN_EPS)
        bound = rule(ref, t32)
        level = EPS32 * 1000.0 ** 2 / 1.0 * float(ref.abs().max())
        assert bound < level / 10, (R, C, bound, level)
        assert max_dev(one_pass_layer_norm32(x, w, b, LN_EPS), ref) > bound, (R, C)


def test_mean1000_rule_separates_one_pass_batchnorm():
    for M, C in [(37, 3), (300, 65)]:
        x, w, b = regime_input("mean1000", M, C, 1), uni(C, seed=2) + 1.5, uni(C, seed=3)
        ref = F.batch_norm(x.double(), None, None, w.double(), b.double(), True, MOM, BN_EPS)
        t32 = F.batch_norm(x, None, None, w, b, True, MOM, BN_EPS)
        bound = rule(ref, t32)
        level = EPS32 * 1000.0 ** 2 / 1.0 * float(ref.abs().max())
        assert bound < level / 10, (M, C, bound, level)
        mean = x.mean(0)
        one_pass = (x - mean) * torch.rsqrt(((x * x).mean(0) - mean * mean).clamp_min(0) + BN_EPS) * w + b
        assert max_dev(one_pass, ref) > bound, (M, C)


# ------------------------------------------------------------------------------------------ LayerNorm
def ln_reference(x, w, b, dy, dtype):
    xr, wr, br = (t.to(dtype).clone().requires_grad_(True) for t in (x, w, b))
    y = F.layer_norm(xr, (x.shape[1],), wr, br, LN_EPS)
    y.backward(dy.to(dtype))
    return y.detach(), xr.grad, wr.grad, br.grad


@gpu
@pytest.mark.parametrize("regime", ["uniform", "const", "mean1000"])
@pytest.mark.parametrize("C", [1, 3, 63, 64, 65, 130, 512])
@pytest.mark.parametrize("R", [1, 5, 9, 100])
def test_layernorm_strided(L, R, C, regime):
    shape = f"R={R},C={C},{regime}"
    x, w, b, dy = regime_input(regime, R, C, 11), uni(C, seed=12) + 1.5, uni(C, seed=13), uni(R, C, seed=14)
    res, d0, p0 = uni(R, C, seed=15), uni(R, C, seed=16), uni(2 * C, seed=17)
    y64, dx64, dw64, db64 = ln_reference(x, w, b, dy, torch.float64)
    y32 = dx32 = dw32 = db32 = None      # torch's fp32 results: the mean-1000 rule's yardstick only
    if regime == "mean1000":
        y32, dx32, dw32, db32 = ln_reference(x, w, b, dy, torch.float32)
    ldx, ldy, lddy, lddx, ldr = C + 3, C + 5, C + 2, C + 4, C + 6
    xp, dyp, rp = Poisoned(x, ld=ldx), Poisoned(dy, ld=lddy), Poisoned(res, ld=ldr)
    wd, bd = w.to(DEV), b.to(DEV)
    y, mean, rstd = Guarded(R, C, ld=ldy), Guarded(1, R), Guarded(1, R)
    assert L.vc_layernorm_fwd(R, C, xp.ptr, ldx, P(wd), P(bd), LN_EPS, y.ptr, ldy, mean.ptr, rstd.ptr, S()) == 0
    check("layernorm_fwd y", shape, y.check(), y64, 1e-5, regime, y32)
    xd = x.double()
    within("layernorm_fwd mean", shape, rel_err(mean.check()[0].numpy(), xd.mean(1).numpy()), 1e-5)
    within("layernorm_fwd rstd", shape,
           rel_err(rstd.check()[0].numpy(), torch.rsqrt(xd.var(1, unbiased=False) + LN_EPS).numpy()), 1e-5)
    if regime == "const":   # variance 0 exactly: rstd = eps^-1/2, y = b
        assert torch.equal(y.check()[0], b) and torch.equal(y.check()[R - 1], b)

    # the partial workspace exactly as large as the plan of 8-row blocks needs, guarded
    part_n = -(-R // 8) * 2 * C
    forms = [("adjacent", 0.0, 0.0), ("separate", 0.5, 1.0), ("dw null", 0.0, 1.0), ("db null", 0.5, 0.0)]
    for form, beta_dx, beta_w in forms:
        dx = Guarded(R, C, ld=lddx, init=d0 if beta_dx else None)
        both = Guarded(1, 2 * C, init=p0 if beta_w else None)
        gw, gb = (Guarded(1, C, init=p0[:C] if beta_w else None), Guarded(1, C, init=p0[C:] if beta_w else None))
        if form == "adjacent":
            dwp, dbp = both.ptr, both.ptr + 4 * C
        else:
            dwp, dbp = (gw.ptr if form != "dw null" else None), (gb.ptr if form != "db null" else None)
        part = Guarded(1, part_n)
        assert L.vc_layernorm_bwd(R, C, dyp.ptr, lddy, xp.ptr, ldx, P(wd), mean.ptr, rstd.ptr, dx.ptr, lddx, beta_dx,
                                  dwp, dbp, beta_w, part.ptr, part_n, S()) == 0
        part.check()
        tag = f"layernorm_bwd[{form}]"
        check(tag + " dx", shape, dx.check() - beta_dx * d0, dx64, 1e-4, regime, dx32)
        got_both, got_w, got_b = both.check()[0], gw.check()[0], gb.check()[0]
        if form == "adjacent":
            got_w, got_b = got_both[:C], got_both[C:]
        else:       # the buffers not passed are as they were
            assert torch.equal(got_both, p0) if beta_w else torch.isnan(got_both).all()
        if form != "dw null":
            check(tag + " dw", shape, got_w - beta_w * p0[:C], dw64, 1e-4, regime, dw32)
        else:
            assert torch.equal(got_w, p0[:C])
        if form != "db null":
            check(tag + " db", shape, got_b - beta_w * p0[C:], db64, 1e-4, regime, db32)
        else:
            assert torch.isnan(got_b).all()

    # dx = res + LN gradient, res untouched; and the split form, bit-identical to vc_layernorm_bwd
    outs = []
    for variant in ("bwd", "res", "split"):
        dx = Guarded(R, C, ld=lddx, init=res if variant == "bwd" else None)
        both, part = Guarded(1, 2 * C, init=p0), Guarded(1, part_n)
        if variant == "bwd":
            assert L.vc_layernorm_bwd(R, C, dyp.ptr, lddy, xp.ptr, ldx, P(wd), mean.ptr, rstd.ptr, dx.ptr, lddx, 1.0,
                                      both.ptr, both.ptr + 4 * C, 1.0, part.ptr, part_n, S()) == 0
        elif variant == "res":
            assert L.vc_layernorm_bwd_res(R, C, dyp.ptr, lddy, xp.ptr, ldx, P(wd), mean.ptr, rstd.ptr, rp.ptr, ldr,
                                          dx.ptr, lddx, both.ptr, both.ptr + 4 * C, 1.0, part.ptr, part_n, S()) == 0
        else:
            assert L.vc_layernorm_bwd_dx(R, C, dyp.ptr, lddy, xp.ptr, ldx, P(wd), mean.ptr, rstd.ptr, rp.ptr, ldr,
                                         dx.ptr, lddx, 0.0, part.ptr, part_n, S()) == 0
            assert L.vc_layernorm_bwd_params(R, C, part.ptr, part_n, both.ptr, both.ptr + 4 * C, 1.0, S()) == 0
        part.check()
        outs.append((dx.check(), both.check()))
    for o in outs[1:]:
        assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1])
    check("layernorm_bwd_res dx", shape, outs[1][0] - res, dx64, 1e-4, regime, dx32)


@gpu
def test_layernorm_small_workspace_doubles_rows(L):
    """512 floats at (R, C) = (100, 64): 13 blocks of 8 rows need 1664, 7 of 16 need 896, 4 of 32 fit exactly
    (ln_partial_rows doubles twice); the guard behind the 512 floats stays untouched and the split form agrees"""
    R, C, n = 100, 64, 512
    x, w, dy = regime_input("uniform", R, C, 21), uni(C, seed=22) + 1.5, uni(R, C, seed=24)
    _, dx64, dw64, db64 = ln_reference(x, w, torch.zeros(C), dy, torch.float64)
    xp, dyp, wd = Poisoned(x, ld=C + 3), Poisoned(dy, ld=C + 2), w.to(DEV)
    mean, rstd = x.double().mean(1), torch.rsqrt(x.double().var(1, unbiased=False) + LN_EPS)
    md, rd = mean.float().to(DEV), rstd.float().to(DEV)
    outs = []
    for split in (False, True):
        dx, gw, gb, part = Guarded(R, C, ld=C + 4), Guarded(1, C), Guarded(1, C), Guarded(1, n)
        if split:
            assert L.vc_layernorm_bwd_dx(R, C, dyp.ptr, C + 2, xp.ptr, C + 3, P(wd), P(md), P(rd), None, 0, dx.ptr, C + 4,
                                         0.0, part.ptr, n, S()) == 0
            assert L.vc_layernorm_bwd_params(R, C, part.ptr, n, gw.ptr, gb.ptr, 0.0, S()) == 0
        else:
            assert L.vc_layernorm_bwd(R, C, dyp.ptr, C + 2, xp.ptr, C + 3, P(wd), P(md), P(rd), dx.ptr, C + 4, 0.0, gw.ptr,
                                      gb.ptr, 0.0, part.ptr, n, S()) == 0
        got_part = part.check()[0]
        assert not torch.isnan(got_part).any()    # 4 blocks x 2 C: every float of the 512 is a partial
        outs.append((dx.check(), gw.check()[0], gb.check()[0]))
    for a_, b_ in zip(*outs):
        assert torch.equal(a_, b_)
    within("layernorm_bwd ws=512 dx", "R=100,C=64", rel_err(outs[0][0].numpy(), dx64.numpy()), 1e-4)
    within("layernorm_bwd ws=512 dw", "R=100,C=64", rel_err(outs[0][1].numpy(), dw64.numpy()), 1e-4)
    within("layernorm_bwd ws=512 db", "R=100,C=64", rel_err(outs[0][2].numpy(), db64.numpy()), 1e-4)


# ------------------------------------------------------------------------------------------ BatchNorm
def bn_reference(x, w, b, rm, rv, dy, train, mask, dtype):
    """y (before the ReLU), the running statistics after the call, and the gradients for dy * mask"""
    xr, wr, br = (t.to(dtype).clone().requires_grad_(True) for t in (x, w, b))
    rm_, rv_ = rm.to(dtype).clone(), rv.to(dtype).clone()
    y = F.batch_norm(xr, rm_, rv_, wr, br, bool(train), MOM, BN_EPS)
    y.backward((dy * mask).to(dtype))
    return y.detach(), rm_, rv_, xr.grad, wr.grad, br.grad


@gpu
@pytest.mark.parametrize("regime", ["uniform", "mean1000"])
@pytest.mark.parametrize("train", [1, 0])
@pytest.mark.parametrize("C", [1, 3, 63, 65, 200])
@pytest.mark.parametrize("M", [2, 37, 65, 300])
def test_batchnorm_strided(L, ws, cnt, M, C, train, regime):
    """At M = 2 the train-mode dx is (dy1 - dy2) / 2 * w * invstd * eps / (var + eps): with a spread far above
    sqrt(eps) it is the residual of a cancellation to ~1e-5 of its terms, which no fp32 BatchNorm holds to 1e-4 of
    the residual (measured with x ~ U(-3, 3): 1e-4 .. 9e-3 here, and torch's fp32 CPU kernel likewise), so the
    uniform M = 2 train-mode input is scaled to a spread of the order of sqrt(eps), where the gradient is well
    conditioned; eval mode (dx = dy w invstd, no cancellation) keeps U(-3, 3) + 0.5."""
    shape = f"M={M},C={C},train={train},{regime}"
    x, w, b, dy = regime_input(regime, M, C, 31), uni(C, seed=32) + 1.5, uni(C, seed=33), uni(M, C, seed=34)
    if M == 2 and train and regime == "uniform":
        x = x * 0.002
    rm0 = uni(C, seed=35) * 0.1 + (1000.0 if regime == "mean1000" else 0.5)
    rv0 = uni(C, seed=36).abs() + 0.5
    d0, p0 = uni(M, C, seed=37), uni(2 * C, seed=38)
    ones = torch.ones(M, C)
    y64, rm64, rv64, dx64, dw64, db64 = bn_reference(x, w, b, rm0, rv0, dy, train, ones, torch.float64)
    need32 = regime == "mean1000"        # torch's fp32 results: the mean-1000 rule's yardstick only
    y32, _, _, dx32, dw32, db32 = (bn_reference(x, w, b, rm0, rv0, dy, train, ones, torch.float32) if need32
                                   else (None,) * 6)
    ldx, ldy, lddy, lddx, ldo = C + 3, C + 5, C + 2, C + 4, C + 6
    xp, dyp = Poisoned(x, ld=ldx), Poisoned(dy, ld=lddy)
    wd, bd = w.to(DEV), b.to(DEV)
    xd = x.double()
    if train:
        mean64, inv64 = xd.mean(0), torch.rsqrt(xd.var(0, unbiased=False) + BN_EPS)
    else:
        mean64, inv64 = rm0.double(), torch.rsqrt(rv0.double() + BN_EPS)

    # forward: stats + apply, forward, forward_ex with counters, stats_ex with counters; with and without ReLU
    outs = []
    for mode in ("split", "forward", "forward_ex", "stats_ex"):
        relu = int(mode != "split")
        y = Guarded(M, C, ld=ldo if relu else ldy)
        mean, inv, rm, rv = Guarded(1, C), Guarded(1, C), Guarded(1, C, init=rm0), Guarded(1, C, init=rv0)
        st = (train, M, C, xp.ptr, ldx, BN_EPS, MOM, mean.ptr, inv.ptr, rm.ptr, rv.ptr)
        if mode == "split" or mode == "stats_ex":
            if mode == "split":
                assert L.vc_bn_stats(*st, P(ws), ws.numel(), S()) == 0
            else:
                assert L.vc_bn_stats_ex(*st, P(ws), ws.numel(), P(cnt), cnt.numel(), S()) == 0
            assert L.vc_bn_apply(M, C, xp.ptr, ldx, mean.ptr, inv.ptr, P(wd), P(bd), relu, y.ptr, y.ld, S()) == 0
        elif mode == "forward":
            assert L.vc_bn_forward(*st, P(wd), P(bd), relu, y.ptr, y.ld, P(ws), ws.numel(), S()) == 0
        else:
            assert L.vc_bn_forward_ex(*st, P(wd), P(bd), relu, y.ptr, y.ld, P(ws), ws.numel(), P(cnt), cnt.numel(),
                                      S()) == 0
        got = [t.check() for t in (y, mean, inv, rm, rv)]
        assert int(cnt.abs().sum()) == 0
        tag = f"bn[{mode}]"
        check(tag + " y", shape, got[0], torch.relu(y64) if relu else y64, 1e-5, regime,
              (torch.relu(y32) if relu else y32) if need32 else None)
        within(tag + " save_mean", shape, rel_err(got[1][0].numpy(), mean64.numpy()), 1e-5)
        within(tag + " save_invstd", shape, rel_err(got[2][0].numpy(), inv64.numpy()), 1e-5)
        within(tag + " running_mean", shape, rel_err(got[3][0].numpy(), rm64.numpy()), 1e-5)
        within(tag + " running_var", shape, rel_err(got[4][0].numpy(), rv64.numpy()), 1e-5)
        outs.append(got)
    for o in outs[2:]:    # the three ReLU forms agree bit for bit
        for a_, b_ in zip(outs[1], o):
            assert torch.equal(a_, b_)
    relu_y = outs[1][0]
    md, idv = outs[0][1][0].to(DEV), outs[0][2][0].to(DEV)

    # backward without a ReLU: overwrite; the statistics are the kernel's own saved ones
    dx, gw, gb = Guarded(M, C, ld=lddx), Guarded(1, C), Guarded(1, C)
    assert L.vc_bn_bwd(train, M, C, dyp.ptr, lddy, xp.ptr, ldx, None, 0, P(md), P(idv), P(wd), dx.ptr, lddx, 0.0, gw.ptr,
                       gb.ptr, 0.0, P(ws), ws.numel(), S()) == 0
    check("bn_bwd dx", shape, dx.check(), dx64, 1e-4, regime, dx32)
    check("bn_bwd dw", shape, gw.check()[0], dw64, 1e-4, regime, dw32)
    check("bn_bwd db", shape, gb.check()[0], db64, 1e-4, regime, db32)

    # through the ReLU: its decisions read from the forward's output (ld ldo), accumulate with beta 1; then
    # recomputed from the affine (bit-identical); then without dx, with counters
    mask = (relu_y > 0).float()
    _, _, _, mx64, mw64, mb64 = bn_reference(x, w, b, rm0, rv0, dy, train, mask, torch.float64)
    _, _, _, mx32, mw32, mb32 = (bn_reference(x, w, b, rm0, rv0, dy, train, mask, torch.float32) if need32
                                 else (None,) * 6)
    op = Poisoned(relu_y, ld=ldo)
    souts = []
    for form in ("relu_out", "affine", "no dx"):
        dx = Guarded(M, C, ld=lddx, init=d0)
        both = Guarded(1, 2 * C, init=p0)
        dxp = None if form == "no dx" else dx.ptr
        if form == "affine":
            assert L.vc_bn_bwd_relu_ex(train, M, C, dyp.ptr, lddy, xp.ptr, ldx, P(md), P(idv), P(wd), P(bd), dxp, lddx, 1.0,
                                       both.ptr, both.ptr + 4 * C, 1.0, P(ws), ws.numel(), None, 0, S()) == 0
        else:
            assert L.vc_bn_bwd_ex(train, M, C, dyp.ptr, lddy, xp.ptr, ldx, op.ptr, ldo, P(md), P(idv), P(wd), dxp, lddx,
                                  1.0, both.ptr, both.ptr + 4 * C, 1.0, P(ws), ws.numel(), P(cnt), cnt.numel(), S()) == 0
        souts.append((dx.check(), both.check()[0]))
        assert int(cnt.abs().sum()) == 0
    assert torch.equal(souts[0][0], souts[1][0]) and torch.equal(souts[0][1], souts[1][1])
    assert torch.equal(souts[2][0], d0)       # no dx: untouched
    check("bn_bwd_ex relu dx", shape, souts[0][0] - d0, mx64, 1e-4, regime, mx32)
    for tag, got in (("relu", souts[0][1]), ("relu no-dx", souts[2][1])):
        check(f"bn_bwd_ex {tag} dw", shape, got[:C] - p0[:C], mw64, 1e-4, regime, mw32)
        check(f"bn_bwd_ex {tag} db", shape, got[C:] - p0[C:], mb64, 1e-4, regime, mb32)
