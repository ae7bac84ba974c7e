"""vc_s2eft_patch_gate_fwd on the MI355X against the numpy token rule and the float64 gate (s2eft_patch_cases.py).

Every gated case first meets the condition on the ORACLE: each float64 sigmoid at least 1e-4 from beta (fp32 rounding
of the pre-activation is orders of magnitude below that, so the kernel's mask must equal float64's) and both mask
values present.  Then mask equals the oracle's exactly, xg is bitwise the token value or its product with 0, and the
ungated call returns the numpy tokens bitwise.  Outputs start as NaN inside guard bands that must stay untouched
(helpers.Guarded); inputs sit between NaN poison off 16-B alignment (helpers.Poisoned).

Shapes: rows of 27, 12, 75 and 147 floats (none a multiple of 4 floats from an aligned base); N = 2 (the three slots
of a row meet two bands); one slice per sample (under 1024 output floats) and 2, 5 and 16 slices whose borders cut rows
(a slice forms only the statistics of the bands its rows' gate reads, wrapping at both ends; N = 5 in 2 slices needs
them all); P*P = 81 > 64 (the per-band reduction's tail loop); more than 8 x 4 bands in a slice (the second round of the
band loop) and 700 rows in one slice (the second round of the 512-thread conv loop); near = 1 and C2 = 0.
"""
import numpy as np
import pytest
import torch

from helpers import Guarded, Poisoned
from s2eft_patch_cases import BETA, case, conditioned

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, C1, C2, P), near, seed: the six near = 3 shapes at seed 0, then near = 1, C2 = 0, P*P > 64 and N > 512
CASES = [((3, 6, 1, 3), 3, 0), ((2, 9, 2, 2), 3, 0), ((3, 1, 1, 5), 3, 0), ((2, 144, 1, 7), 3, 0),
         ((5, 30, 1, 7), 3, 0), ((2, 300, 1, 1), 3, 0), ((3, 7, 1, 3), 1, 0), ((2, 20, 1, 9), 1, 0),
         ((3, 10, 0, 3), 3, 0), ((2, 5, 0, 9), 3, 0), ((2, 37, 0, 2), 1, 0), ((2, 700, 0, 1), 1, 0)]
IDS = [f"{s[0]}x{s[1]}+{s[2]}x{s[3]}-near{n}" for s, n, _ in CASES]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vitcnn_amd._lib import lib
    return lib()


def S():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _inputs(c, lead):
    """the two patches between NaN poison, `lead` floats off the allocation's alignment"""
    B = c["x1"].shape[0]
    x1 = Poisoned(torch.from_numpy(c["x1"]).reshape(B, -1), lead=lead)
    x2 = Poisoned(torch.from_numpy(c["x2"]).reshape(B, -1), lead=(lead + 1) % 4) if c["x2"] is not None else None
    return x1, x2


@pytest.mark.parametrize("shape,near,seed", CASES, ids=IDS)
def test_patch_gate(L, shape, near, seed):
    c = case(shape, seed, near)
    conditioned(c)                                   # on the oracle, before the kernel is looked at
    B, C1, C2, P = shape
    N, C = C1 + C2, near * P * P
    x1, x2 = _inputs(c, lead=1)
    w, bias = torch.from_numpy(c["w"]).to(DEV), torch.from_numpy(c["bias"]).to(DEV)
    xg, mask = Guarded(B * N, C, lead=3), Guarded(B, N, lead=1)
    assert L.vc_s2eft_patch_gate_fwd(B, C1, C2, P, near, x1.ptr, x2.ptr if x2 else None, w.data_ptr(), bias.data_ptr(),
                                     BETA, xg.ptr, mask.ptr, S()) == 0
    got_mask, got_xg = mask.check().numpy(), xg.check().numpy().reshape(B, N, C)
    print(f"PATCH_GATE {shape} near {near}: margin {c['margin']:.2e}, ones {c['ones']:.2f}")
    assert np.array_equal(got_mask, c["mask"])
    want = c["tokens"] * c["mask"][:, :, None]       # x * 1 = x, x * 0 = +-0: the kernel's own product
    assert np.array_equal(bits(got_xg), bits(want))


@pytest.mark.parametrize("shape,near,seed", CASES, ids=IDS)
def test_patch_gate_ungated(L, shape, near, seed):
    """w null: xg is the token rows bitwise; mask is optional and all ones"""
    c = case(shape, seed, near)
    B, C1, C2, P = shape
    N, C = C1 + C2, near * P * P
    x1, x2 = _inputs(c, lead=2)
    for with_mask in (False, True):
        xg, mask = Guarded(B * N, C, lead=1), Guarded(B, N)
        assert L.vc_s2eft_patch_gate_fwd(B, C1, C2, P, near, x1.ptr, x2.ptr if x2 else None, None, None, 0.0, xg.ptr,
                                         mask.ptr if with_mask else None, S()) == 0
        assert np.array_equal(bits(xg.check().numpy().reshape(B, N, C)), bits(c["tokens"]))
        if with_mask:
            assert np.array_equal(mask.check().numpy(), np.ones((B, N), dtype=np.float32))


def test_patch_gate_equals_the_gate_on_materialised_tokens(L):
    """the config-5 shape: vc_s2eft_patch_gate_fwd(x1, x2) and vc_s2eft_gate_fwd(tokens) give the same mask and xg"""
    shape = (2, 144, 1, 7)
    c = case(shape, 0)
    conditioned(c)
    B, C1, C2, P = shape
    N, C = C1 + C2, 3 * P * P
    dev = {k: torch.from_numpy(c[k]).to(DEV) for k in ("x1", "x2", "w", "bias", "tokens")}
    out = [(torch.empty(B, N, C, device=DEV), torch.empty(B, N, device=DEV)) for _ in range(2)]
    L.vc_s2eft_patch_gate_fwd(B, C1, C2, P, 3, dev["x1"].data_ptr(), dev["x2"].data_ptr(), dev["w"].data_ptr(),
                              dev["bias"].data_ptr(), BETA, out[0][0].data_ptr(), out[0][1].data_ptr(), S())
    L.vc_s2eft_gate_fwd(B, N, C, dev["tokens"].data_ptr(), dev["w"].data_ptr(), dev["bias"].data_ptr(), BETA,
                        out[1][0].data_ptr(), out[1][1].data_ptr(), S())
    torch.cuda.synchronize()
    assert torch.equal(out[0][1], out[1][1])
    assert np.array_equal(bits(out[0][0].cpu().numpy()), bits(out[1][0].cpu().numpy()))


def test_neighbour_band_tokens_helper(L):
    from vitcnn_amd.s2eft import neighbour_band_tokens
    for shape, near in (((3, 6, 1, 3), 3), ((2, 20, 1, 9), 1)):
        c = case(shape, 0, near)
        got = neighbour_band_tokens(torch.from_numpy(c["x1"]).to(DEV), torch.from_numpy(c["x2"]).to(DEV), near)
        assert got.is_cuda and got.dtype == torch.float32
        assert np.array_equal(bits(got.cpu().numpy()), bits(c["tokens"]))
    with pytest.raises(RuntimeError):
        neighbour_band_tokens(torch.zeros(2, 3, 3, 3), torch.zeros(2, 1, 3, 3))
