"""S2EFT over the two patches, the parts that need no GPU: the numpy token rule against explicit
loops, the new entry point in the header and its host-side refusals, `get_model("S2EFT")` building the two-input class
with `ViT`'s parameter tree, the captured step accepting it, and the forward's shape checks."""
import ctypes

import numpy as np
import pytest
import torch

from s2eft_patch_cases import case, gate_sigmoid, tokens

KW = dict(image_size=3, near_band=3, num_patches=6, num_classes=5, dim=16, depth=3, heads=2, mlp_dim=8, mode="CAF")


def test_token_rule_equals_explicit_loops():
    B, C1, C2, P, near = 2, 5, 1, 3, 3
    rng = np.random.default_rng(1)
    x1 = rng.standard_normal((B, C1, P, P)).astype(np.float32)
    x2 = rng.standard_normal((B, C2, P, P)).astype(np.float32)
    N, PP = C1 + C2, P * P
    want = np.full((B, N, near * PP), np.nan, dtype=np.float32)
    for b in range(B):
        for j in range(N):
            for s in range(near):
                n = (j + s - near // 2) % N
                src = x1[b, n] if n < C1 else x2[b, n - C1]
                want[b, j, s * PP:(s + 1) * PP] = src.reshape(-1)      # p = row * P + col: the NCHW order
    got = tokens(x1, x2, near)
    assert got.dtype == np.float32 and got.shape == (B, N, near * PP) and np.array_equal(got, want)
    # the wrap, by value: band 0's previous band is the LiDAR band, the LiDAR band's next band is HSI band 0
    assert np.array_equal(got[:, 0, :PP], x2[:, 0].reshape(B, PP))
    assert np.array_equal(got[:, 0, PP:2 * PP], x1[:, 0].reshape(B, PP))
    assert np.array_equal(got[:, 0, 2 * PP:], x1[:, 1].reshape(B, PP))
    assert np.array_equal(got[:, N - 1, :PP], x1[:, C1 - 1].reshape(B, PP))
    assert np.array_equal(got[:, N - 1, PP:2 * PP], x2[:, 0].reshape(B, PP))
    assert np.array_equal(got[:, N - 1, 2 * PP:], x1[:, 0].reshape(B, PP))
    # near = 1 is the plain view; C2 = 0 wraps inside the HSI bands
    assert np.array_equal(tokens(x1, x2, 1), np.concatenate([x1, x2], 1).reshape(B, N, PP))
    assert np.array_equal(tokens(x1, None, 3)[:, 0, :PP], x1[:, C1 - 1].reshape(B, PP))


def test_float64_gate_equals_torch_conv1d():
    c = case((3, 6, 1, 3), 0)
    t = torch.from_numpy(c["tokens"]).double()
    g = torch.stack([t.mean(2), t.amax(2)], 1)
    ref = torch.sigmoid(torch.nn.functional.conv1d(g, torch.from_numpy(c["w"]).double(),
                                                   torch.from_numpy(c["bias"]).double(), padding=3))[:, 0]
    assert np.allclose(gate_sigmoid(c["tokens"], c["w"], c["bias"]), ref.numpy(), rtol=0, atol=1e-14)
    assert c["margin"] >= 1e-4 and 0.0 < c["ones"] < 1.0


def test_header_declares_the_patch_gate():
    from vitcnn_amd._lib import parse_header
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    #                                            B  C1 C2 P  near x1 x2 w  bias beta xg mask stream
    assert parse_header()["vc_s2eft_patch_gate_fwd"] == [i, i, i, i, i, p, p, p, p, f, p, p, p]


REFUSED = [
    ("B = 0", (0, 6, 1, 3, 3)),
    ("C1 = 0", (2, 0, 1, 3, 3)),
    ("C2 < 0", (2, 6, -1, 3, 3)),
    ("P = 0", (2, 6, 1, 0, 3)),
    ("near = 2", (2, 6, 1, 3, 2)),
    ("near = 5", (2, 6, 1, 3, 5)),
    ("near = 0", (2, 6, 1, 3, 0)),
    ("C1 + C2 = 4097", (2, 4096, 1, 3, 3)),
    ("C1 + C2 overflows int", (2, 2 ** 31 - 1, 2 ** 31 - 1, 1, 1)),
    ("N * near * P * P = 2^31", (2, 2048, 0, 1024, 1)),
    ("P * P overflows int", (2, 1, 0, 65536, 1)),
    ("x2 null with C2 = 1", (2, 6, 1, 3, 3)),
]


@pytest.mark.parametrize("what,shape", REFUSED, ids=[r[0] for r in REFUSED])
def test_patch_gate_refusals(what, shape):
    """vc_s2eft_patch_gate_fwd returns non-zero before any launch: the null pointers are never touched"""
    from vitcnn_amd._lib import lib
    assert lib().raw["vc_s2eft_patch_gate_fwd"](*shape, None, None, None, None, 0.4, None, None, None) != 0, what


def test_get_model_builds_the_two_input_class_with_vits_parameters():
    from vitcnn_amd import S2EFT
    from vitcnn_amd.model_utils import get_model
    from vitcnn_amd.s2eft import ViT
    torch.manual_seed(4)
    m, opt, crit, kw = get_model("S2EFT", n_classes=6, n_bands=(10, 1), ignored_labels=[0], dataset="synthetic",
                                 patch_size=3, device=torch.device("cpu"))
    assert type(m) is S2EFT and isinstance(m, ViT)
    assert m.N == 11 and m.C == 27 and m.near == 3 and m.image_size == 3
    torch.manual_seed(4)
    v = ViT(image_size=3, near_band=3, num_patches=10, num_classes=6, dim=64, depth=5, heads=4, mlp_dim=8, dropout=0.1,
            emb_dropout=0.1, mode="CAF")
    a, b = m.state_dict(), v.state_dict()
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert m._poff == v._poff


def test_captured_step_accepts_s2eft_and_still_refuses_vit():
    from vitcnn_amd import AdamW, CrossEntropyLoss, S2EFT
    from vitcnn_amd.s2eft import ViT
    from vitcnn_amd.step import TrainStepper
    m = S2EFT(**KW)
    st = TrainStepper(m, AdamW(m.parameters(), lr=1e-4), CrossEntropyLoss(), capture_step=True)
    assert st.generic and st.launch == "hipGraph"
    one = ViT(**KW)
    st = TrainStepper(one, AdamW(one.parameters(), lr=1e-4), CrossEntropyLoss(), capture_step=True)
    assert not st.generic and "two inputs" in st.launch


def test_forward_refuses_what_it_cannot_run():
    from vitcnn_amd import S2EFT
    m = S2EFT(**KW)
    x1, x2 = torch.zeros(2, 6, 3, 3), torch.zeros(2, 1, 3, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x1, x2)
    with pytest.raises(NotImplementedError):
        m(x1, x2, mask=torch.ones(2, 7))
    # the shape checks come after the device check (_shape_check: the inputs claim a cuda device)
    for a, b in (((2, 5, 3, 3), (2, 1, 3, 3)), ((2, 6, 3, 3), (2, 2, 3, 3)), ((2, 6, 5, 5), (2, 1, 5, 5)),
                 ((2, 6, 3, 3), (2, 1, 3, 2)), ((2, 6, 3, 3), (3, 1, 3, 3)), ((2, 7, 9), (2, 1, 3, 3))):
        with pytest.raises(RuntimeError, match=r"expected x1 \[B, C1, 3, 3\]"):
            _shape_check(m, torch.zeros(*a), torch.zeros(*b))
    with pytest.raises(ValueError):
        S2EFT(**dict(KW, near_band=5))


def _shape_check(m, x1, x2):
    """S2EFT.forward behind its device check (no GPU here): the inputs claim a cuda device"""
    class _Dev:
        type = "cuda"

    class _T:
        def __init__(self, t):
            self.t, self.device, self.shape = t, _Dev(), t.shape

        def dim(self):
            return self.t.dim()

    return m.forward(_T(x1), _T(x2))
