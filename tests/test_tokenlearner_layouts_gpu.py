"""The TokenLearner kernels (vc_tl_pixel_stats / vc_tl_fwd / vc_tl_relu_mask / vc_tl_bwd, tokenlearner.hip) off the
models' shapes, on the MI355X: channel counts that are no multiple of 4 (1, 3, 63, 70, 130) and one that is (64), x
rows of leading dimension C, C + 4 and C + 3, dx rows of C + 5, x or dZ one float off 16 B.  vc_tl_bwd reads the x and
dZ rows by 16-B loads only where C % 4 == 0, ldx % 4 == 0 and both bases are aligned (tl_bwd_da<true> /
tl_bwd_dx<true>); every other case here takes the guarded-load templates, which the older tests reach only through
whole models.

The yardstick is that of tests/test_tokenlearner_gpu.py (its helpers are imported, its bounds unchanged): the HIP path's
pooled values and ReLU decisions, float64 after that; uniform and ill-conditioned inputs, train and eval.  x, dZ and the
parameters are helpers.Poisoned; every output, the running statistics and the fp64 scratch are helpers.Guarded, and
dparams, a, Z, dx and stats start as NaN.

At C = 64 the guarded-load kernels (ldx = C + 3, or a base off 16 B) read the same values as the 16-B-load kernels and
feed them to the same MFMA sequence: their dx and dparams are bit-identical to the aligned call's, which
test_guarded_loads_agree_with_vector_loads asserts besides the float64 bound.
"""
import pytest
import torch

from helpers import Guarded, Poisoned, within
from test_tokenlearner_gpu import EPS32, _buffers, _input, _params, _reference

gpu = pytest.mark.gpu
SHAPES = [(3, 9, 1, 4), (2, 25, 3, 9), (3, 49, 63, 25), (2, 81, 70, 49), (2, 49, 64, 25), (2, 16, 130, 4)]
# name -> (ldx - C, lead of x, lead of dZ)
LAYOUTS = {"nat": (0, 0, 0), "pad4": (4, 0, 0), "pad3": (3, 0, 0), "x1": (0, 1, 0), "dz1": (0, 0, 1)}


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vitcnn_amd._lib import lib
    return lib()


def _s():
    return torch.cuda.current_stream().cuda_stream


def run_hip(L, train, x, B, HW, C, S, par, buf, dZ, layout):
    """pixel_stats -> fwd -> relu_mask -> bwd over placed operands; every guard checked"""
    pad, leadx, leaddz = LAYOUTS[layout]
    M, ldx, lddx = B * HW, C + pad, C + 5
    xp, dzp, pp = Poisoned(x, ld=ldx, lead=leadx), Poisoned(dZ.view(B * S, C), lead=leaddz), Poisoned(par.reshape(1, -1))
    bufd = Guarded(1, 2 * S, init=buf.reshape(1, -1))
    mx, avg, amx = Guarded(1, M), Guarded(1, M), Guarded(1, M, dtype=torch.int32)
    ws = Guarded(1, (L.vc_tl_ws_floats(B, HW, S) + 1) // 2, dtype=torch.float64)
    st = Guarded(1, 2 * S + 8, dtype=torch.float64)
    a, Z, mask = Guarded(B * S, HW), Guarded(B * S, C), Guarded(B * S, HW, dtype=torch.uint8)
    dx, gp = Guarded(M, C, ld=lddx), Guarded(S, 5)
    assert L.vc_tl_pixel_stats(M, C, xp.ptr, ldx, mx.ptr, amx.ptr, avg.ptr, ws.ptr, _s()) == 0
    assert L.vc_tl_fwd(train, B, HW, C, S, xp.ptr, ldx, mx.ptr, avg.ptr, pp.ptr, bufd.ptr, 1e-5, 0.1, ws.ptr, st.ptr,
                       a.ptr, Z.ptr, _s()) == 0
    assert L.vc_tl_relu_mask(B, HW, S, mx.ptr, avg.ptr, pp.ptr, st.ptr, mask.ptr, _s()) == 0
    assert L.vc_tl_bwd(train, B, HW, C, S, xp.ptr, ldx, mx.ptr, avg.ptr, amx.ptr, pp.ptr, st.ptr, a.ptr, dzp.ptr, ws.ptr,
                       dx.ptr, lddx, gp.ptr, _s()) == 0
    ws.check()
    return dict(mx=mx.check()[0], amx=amx.check()[0].long(), avg=avg.check()[0], st=st.check()[0], a=a.check().reshape(-1),
                Z=Z.check().reshape(-1), mask=mask.check().reshape(-1).bool(), dx=dx.check(), gp=gp.check(),
                buf=bufd.check().view(S, 2))


def ratio(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def case(B, HW, C, S, regime, train):
    x = _input(B, HW, C, seed=B * 131 + C, regime=regime)
    par = _params(S, seed=S)
    buf = _buffers(x, par, S, regime, train)
    dZ = torch.rand(B * S * C, generator=torch.Generator().manual_seed(7)) * 2 - 1
    return x, par, buf, dZ


def judge(hip, x, par, buf, dZ, B, HW, C, S, train, shape):
    """the assertions of tests/test_tokenlearner_gpu.py, the measured figures printed"""
    assert torch.equal(hip["mx"], x.max(1).values)
    assert torch.equal(hip["amx"], x.argmax(1)) or bool((x.gather(1, hip["amx"][:, None])[:, 0] == hip["mx"]).all())
    within("tl_pixel_stats avg", shape, float((hip["avg"].double() - x.double().mean(1)).abs().max()),
           1e-6 * float(x.abs().max()), inclusive=True)
    ref = _reference(train, x, B, HW, C, S, par, buf, dZ, hip)
    st = hip["st"]
    assert torch.allclose(st[0:2 * S:2], ref["mean"], rtol=1e-12, atol=1e-14 * float(ref["mean"].abs().max()))
    assert torch.allclose(st[1:2 * S:2], 1.0 / torch.sqrt(ref["var"] + EPS32), rtol=1e-9)
    assert abs(float(st[2 * S]) - B * HW) == 0
    within("tl_fwd a", shape, ratio(hip["a"], ref["a"]), 1e-6, inclusive=True)
    within("tl_fwd Z", shape, ratio(hip["Z"], ref["Z"]), 1e-5, inclusive=True)
    if train:
        within("tl_fwd running statistics", shape, ratio(hip["buf"], ref["buf"]), 1e-6, inclusive=True)
    else:
        assert torch.equal(hip["buf"], buf)
    gref = ref["gp"]
    floor = 1e-7 * float(gref.abs().max())
    for j in range(5):
        err = float((hip["gp"][:, j].double() - gref[:, j]).abs().max())
        within(f"tl_bwd dparams[:, {j}] (abs)", shape, err, 1e-5 * float(gref[:, j].abs().max()) + floor, inclusive=True)
    within("tl_bwd dx", shape, ratio(hip["dx"], ref["dx"]), 1e-5, inclusive=True)


@gpu
@pytest.mark.parametrize("train", [1, 0])
@pytest.mark.parametrize("regime", ["uniform", "illcond"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("B,HW,C,S", SHAPES)
def test_tokenlearner_layouts(L, B, HW, C, S, layout, regime, train):
    x, par, buf, dZ = case(B, HW, C, S, regime, train)
    hip = run_hip(L, train, x, B, HW, C, S, par, buf, dZ, layout)
    judge(hip, x, par, buf, dZ, B, HW, C, S, train, f"B={B},HW={HW},C={C},S={S},{layout},{regime},train={train}")


@gpu
@pytest.mark.parametrize("train", [1, 0])
@pytest.mark.parametrize("regime", ["uniform", "illcond"])
def test_guarded_loads_agree_with_vector_loads(L, regime, train):
    """C = 64: ldx = C + 3 and a base off 16 B take the guarded loads over the same values as the 16-B loads of the
    natural and the ldx = C + 4 layouts -- every output bit-identical"""
    B, HW, C, S = 2, 49, 64, 25
    x, par, buf, dZ = case(B, HW, C, S, regime, train)
    outs = {k: run_hip(L, train, x, B, HW, C, S, par, buf, dZ, k) for k in LAYOUTS}
    for k in ("pad4", "pad3", "x1", "dz1"):
        for name in ("mx", "amx", "avg", "st", "a", "Z", "mask", "dx", "gp", "buf"):
            assert torch.equal(outs[k][name], outs["nat"][name]), (k, name)
