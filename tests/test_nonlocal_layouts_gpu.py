"""vc_nonlocal_attn_fwd / _bwd and vc_nonlocal_attn_pool_fwd / _pool_bwd (attention.hip) off the models' shapes, on
the MI355X, against float64 torch autograd on the CPU over the fp32 inputs widened.

Routes (chosen on the host): with Ci % 4 == 0 and 16-B aligned bases the MFMA forward runs at any key count P <= 16
that is not 4, 9 or 16 (and at those from B = 256), the MFMA backward whenever S <= 256; everything else takes the
wave-per-row kernels, which exist for P in {1, 4, 9, 16} only.  So P in {2, 5, 12, 15} reach the key-tail masks of the
MFMA kernels (4 g + r < P inside a lane group, c < P across lanes), S in {1, 7, 17, 121} their query-tail masks,
S in {257, 289} the backward's fallback, Ci in {6, 70} and a theta one float off 16 B the wave-per-row kernels.

Three regimes.  Uniform inputs: bounds 1e-5 of max |ref| on att and o, 1e-4 on the gradients.  Peaked: one key of
every batch element scores 30 above the rest; steep: 100 above, where exp overflows fp32 unless the row maximum is
subtracted first (at 30 it does not: e^35 fits), run at Ci = 64 and in the smaller tests.  No fixed bound can be derived
for the last two: the max deviation is held to 4 x torch fp32 CPU's deviation from float64 on the same input
+ 2 eps32 max |ref| (test_norm_layouts_gpu.rule; in the steep regime + 2^-126, the smallest normal fp32 number,
because the e^-100 weights are denormals that the GPU may flush to zero and torch's CPU does not).  That rule bites
on att, o and dpooled.  On dtheta it asserts little in these regimes: dtheta is of the order e^-30 there and its
leading term cancels in fp32 (dA - sum att dA, with att = 1 on the peak), so torch's fp32 result -- like the
kernels' -- deviates by about the whole of max |ref|, and the bound is about 4 max |ref|; the uniform regime carries
dtheta.

Inputs are helpers.Poisoned, outputs helpers.Guarded (NaN-initialised: every element must be written).  The pooled
forms are compared with torch.nn.functional.max_pool2d (values and taps bit for bit) and the float64 attention, with
ldpg = 2 Ci + 4 and 2 Ci + 3; where the fused backward runs, dpooled keeps its sentinel bit for bit.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import SENTINEL, Guarded, Poisoned, rel_err, within
from test_kernels_gpu import rnd
from test_norm_layouts_gpu import max_dev, rule

gpu = pytest.mark.gpu
LEGACY_P = (1, 4, 9, 16)      # key counts the wave-per-row kernels are built for
PEAK = {"peaked": 30.0, "steep": 100.0}
FLT_MIN = 2.0 ** -126       # the smallest normal fp32 number


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vitcnn_amd._lib import lib
    return lib()


def S_():
    return torch.cuda.current_stream().cuda_stream


def routes(B, S, P, Ci, aligned=True):
    """(forward, backward) kernel the host picks: the docstring's rule, restated for the figures' labels"""
    vec = Ci % 4 == 0 and aligned
    return ("mfma" if vec and (B >= 256 or P not in (4, 9, 16)) else "wave"), ("mfma" if vec and S <= 256 else "wave")


@functools.lru_cache(maxsize=None)
def inputs(B, S, P, Ci, regime):
    theta, pooled, dout = rnd(B * S, Ci, seed=51), rnd(B * P, 2 * Ci, seed=52), rnd(B * S, Ci, seed=53)
    if regime != "uniform":     # channel 0 adds 30 (100) to key b % P of batch element b and nothing to the others
        theta[:, 1:] /= Ci ** 0.5
        theta[:, 0] = 5.0
        pooled[:, 0] = 0.0
        for b in range(B):
            pooled[b * P + b % P, 0] = PEAK[regime] / 5.0
    return theta, pooled, dout


def attention(theta, pooled, dout, B, S, P, Ci, dtype):
    """(att, o, dtheta, dpooled) of softmax(theta phi^T) g by autograd in dtype"""
    th = theta.to(dtype).view(B, S, Ci).clone().requires_grad_(True)
    pp = pooled.to(dtype).view(B, P, 2 * Ci).clone().requires_grad_(True)
    att = torch.softmax(th @ pp[..., :Ci].transpose(1, 2), dim=-1)
    o = att @ pp[..., Ci:]
    o.backward(dout.to(dtype).view(B, S, Ci))
    return att.detach().reshape(B * S, P), o.detach().reshape(B * S, Ci), th.grad.reshape(B * S, Ci), \
        pp.grad.reshape(B * P, 2 * Ci)


@functools.lru_cache(maxsize=None)
def reference(B, S, P, Ci, regime):
    """float64 results, and torch's fp32 ones where the rule needs them (the peaked and the steep regime)"""
    args = inputs(B, S, P, Ci, regime) + (B, S, P, Ci)
    return attention(*args, torch.float64), (attention(*args, torch.float32) if regime != "uniform" else [None] * 4)


def judge(name, shape, got, ref, bound, t32, floor=0.0):
    if t32 is not None:
        within(name + " (peaked / steep: max abs dev)", shape, max_dev(got, ref), rule(ref, t32) + floor, inclusive=True)
    else:
        within(name, shape, rel_err(got.numpy(), ref.numpy()), bound)


def run_attention(L, B, S, P, Ci, regime, lead=0):
    theta, pooled, dout = inputs(B, S, P, Ci, regime)
    ref, r32 = reference(B, S, P, Ci, regime)
    rf, rb = routes(B, S, P, Ci, lead == 0)
    shape = f"B={B},S={S},P={P},Ci={Ci},lead={lead},{regime}"
    th, pp, dd = Poisoned(theta, lead=lead), Poisoned(pooled), Poisoned(dout)
    att, o = Guarded(B * S, P), Guarded(B * S, Ci)
    dth, dpp = Guarded(B * S, Ci), Guarded(B * P, 2 * Ci)
    assert L.vc_nonlocal_attn_fwd(B, S, P, Ci, th.ptr, pp.ptr, att.ptr, o.ptr, S_()) == 0
    assert L.vc_nonlocal_attn_bwd(B, S, P, Ci, th.ptr, pp.ptr, att.ptr, dd.ptr, dth.ptr, dpp.ptr, S_()) == 0
    # steep: the weights e^-100 of the other keys and everything scaled by them lie below the smallest normal fp32
    # number, which torch's CPU arithmetic keeps as denormals and the GPU's fp32 arithmetic may flush to zero
    floor = FLT_MIN if regime == "steep" else 0.0
    judge(f"nonlocal_attn_fwd[{rf}] att", shape, att.check(), ref[0], 1e-5, r32[0], floor)
    judge(f"nonlocal_attn_fwd[{rf}] o", shape, o.check(), ref[1], 1e-5, r32[1], floor)
    judge(f"nonlocal_attn_bwd[{rb}] dtheta", shape, dth.check(), ref[2], 1e-4, r32[2], floor)
    judge(f"nonlocal_attn_bwd[{rb}] dpooled", shape, dpp.check(), ref[3], 1e-4, r32[3], floor)


REGIMES = ["uniform", "peaked", "steep"]


@gpu
@pytest.mark.parametrize("Ci,regime", [(Ci, r) for Ci in (4, 64, 72) for r in REGIMES if Ci == 64 or r != "steep"])
@pytest.mark.parametrize("S", [1, 7, 16, 17, 81, 121, 256])
@pytest.mark.parametrize("P", [1, 2, 4, 5, 9, 12, 15, 16])
def test_attention_key_and_query_tails(L, P, S, Ci, regime):
    """Ci % 4 == 0, aligned: the MFMA backward everywhere, the MFMA forward at P not in {4, 9, 16}"""
    run_attention(L, 2, S, P, Ci, regime)


@gpu
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("P", [4, 16])
@pytest.mark.parametrize("S", [257, 289])
def test_attention_backward_fallback_past_256_queries(L, S, P, regime):
    run_attention(L, 2, S, P, 64, regime)


@gpu
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("P", LEGACY_P)
@pytest.mark.parametrize("Ci,S,lead", [(6, 7, 0), (70, 81, 0), (64, 17, 1)])
def test_attention_wave_per_row(L, Ci, S, lead, P, regime):
    """Ci % 4 != 0, or theta one float off 16 B at Ci = 64: the wave-per-row kernels both ways"""
    run_attention(L, 2, S, P, Ci, regime, lead)


@gpu
@pytest.mark.parametrize("regime", REGIMES)
def test_attention_mfma_forward_at_a_legacy_key_count(L, regime):
    """B = 256: the MFMA forward at P = 4"""
    run_attention(L, 256, 9, 4, 8, regime)


# ------------------------------------------------------------------------------------------ pooled forms
def pooled_reference(pg, theta, dout, B, Hs, Ci):
    """float64: 2x2 max pool of the phi | g map (values, taps t = 2 dh + dw), the attention over it, and the
    gradients with respect to theta and the unpooled map"""
    S, PW = Hs * Hs, Hs // 2
    P = PW * PW
    pgr = pg.double().clone().requires_grad_(True)
    th = theta.double().view(B, S, Ci).clone().requires_grad_(True)
    maps = pgr.view(B, Hs, Hs, 2 * Ci).permute(0, 3, 1, 2)
    pooled, idx = F.max_pool2d(maps, 2, 2, return_indices=True)          # [B, 2Ci, PW, PW]; idx = h Hs + w
    pp = pooled.permute(0, 2, 3, 1).reshape(B, P, 2 * Ci)
    ih, iw = idx // Hs, idx % Hs
    taps = (2 * (ih % 2) + iw % 2).permute(0, 2, 3, 1).reshape(B * P, 2 * Ci)
    att = torch.softmax(th @ pp[..., :Ci].transpose(1, 2), dim=-1)
    o = att @ pp[..., Ci:]
    o.backward(dout.double().view(B, S, Ci))
    return pp.detach().reshape(B * P, 2 * Ci), taps, att.detach().reshape(B * S, P), o.detach().reshape(B * S, Ci), \
        th.grad.reshape(B * S, Ci), pgr.grad


@gpu
@pytest.mark.parametrize("pad", [4, 3])
@pytest.mark.parametrize("Ci", [64, 70])
@pytest.mark.parametrize("Hs", [2, 3, 5, 6, 8, 9])
def test_pooled_attention(L, Hs, Ci, pad):
    """vc_nonlocal_attn_pool_fwd with ldpg = 2 Ci + pad, then vc_nonlocal_attn_pool_bwd: the fused forward at
    Hs >= 5 (P in {4, 9, 16}, B < 256), the two launches at Hs in {2, 3} (P = 1); the fused backward at Ci = 64,
    the two launches (through dpooled) at Ci = 70"""
    B, S, PW = 2, Hs * Hs, Hs // 2
    P, ldpg = PW * PW, 2 * Ci + pad
    shape = f"B={B},Hs={Hs},Ci={Ci},ldpg={ldpg}"
    pg, theta, dout = rnd(B * S, 2 * Ci, seed=61), rnd(B * S, Ci, seed=62), rnd(B * S, Ci, seed=63)
    ref_pp, ref_taps, ref_att, ref_o, ref_dth, ref_dpg = pooled_reference(pg, theta, dout, B, Hs, Ci)
    pgp, th, dd = Poisoned(pg, ld=ldpg), Poisoned(theta), Poisoned(dout)
    pp, arg = Guarded(B * P, 2 * Ci), Guarded(B * P, 2 * Ci, dtype=torch.uint8)
    att, o = Guarded(B * S, P), Guarded(B * S, Ci)
    assert L.vc_nonlocal_attn_pool_fwd(B, S, P, Ci, Hs, th.ptr, pgp.ptr, ldpg, pp.ptr, arg.ptr, att.ptr, o.ptr, S_()) == 0
    assert torch.equal(pp.check().double(), ref_pp)
    assert torch.equal(arg.check().long(), ref_taps)
    within("nonlocal_attn_pool_fwd att", shape, rel_err(att.check().numpy(), ref_att.numpy()), 1e-5)
    within("nonlocal_attn_pool_fwd o", shape, rel_err(o.check().numpy(), ref_o.numpy()), 1e-5)

    fused = Ci % 4 == 0      # S <= 81 and every base aligned
    dth, dpg = Guarded(B * S, Ci), Guarded(B * S, 2 * Ci)
    dpp = Guarded(B * P, 2 * Ci, init=torch.full((B * P, 2 * Ci), SENTINEL) if fused else None)
    assert L.vc_nonlocal_attn_pool_bwd(B, S, P, Ci, Hs, th.ptr, pp.ptr, att.ptr, dd.ptr, arg.ptr, dth.ptr, dpp.ptr,
                                       dpg.ptr, S_()) == 0
    within("nonlocal_attn_pool_bwd dtheta", shape, rel_err(dth.check().numpy(), ref_dth.numpy()), 1e-4)
    got = dpg.check()
    within("nonlocal_attn_pool_bwd dpg", shape, rel_err(got.numpy(), ref_dpg.numpy()), 1e-4)
    assert torch.equal(got == 0, ref_dpg == 0)        # 0 off the winning taps and in the uncovered last row / column
    if Hs % 2:
        g4 = got.view(B, Hs, Hs, 2 * Ci)
        assert not g4[:, Hs - 1].any() and not g4[:, :, Hs - 1].any()
    if fused:        # the intermediate of the two-launch form is not touched
        assert torch.equal(dpp.check().view(torch.int32), torch.full((B * P, 2 * Ci), SENTINEL).view(torch.int32))
    else:            # ... and there it is the pooled gradient: the non-zero entries of dpg
        win = ref_dpg.view(B, Hs, Hs, 2 * Ci)[:, :2 * PW, :2 * PW].reshape(B, PW, 2, PW, 2, 2 * Ci).sum((2, 4))
        want = win.reshape(B * P, 2 * Ci)
        within("nonlocal_attn_pool_bwd dpooled", shape, rel_err(dpp.check().numpy(), want.numpy()), 1e-4)
