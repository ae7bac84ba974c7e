"""MHST's `conv` option and the vc_mhst_pconv_* family without a GPU: the "mfma" model is the "direct" model (same
state_dict keys and initial values), get_model passes the option through, bad modes raise; vc_mhst_pconv_ok accepts every
site of the model's pyramidal stages and refuses what the family cannot take; vc_mhst_pconv_fwd / _dgrad / _wgrad return 1
on the host, before any launch, for a refused shape, a short workspace, a null or misaligned pointer."""
import pytest
import torch

from mhst_cases import CASES, REGISTRY, build

# (C, O, G, KS, ldx, ldy) of the sites vc_mhst_pconv_ok must accept (hsi_encoder.conv4, lidar_encoder.conv2,
# pyconv_classifier.conv1)
HSI = [(16, 16, g, k, 16, 64) for k, g in zip((3, 5, 7, 9), (1, 2, 4, 8))]
LIDAR = [(32, 16, 1, k, 32, 64) for k in (3, 5, 7, 9)]
CLASSIFIER = [(64, 16, 2, k, 64, 32) for k in (3, 5)]
DEPTHS = (1, 3, 10, 48, 171)


def raw():
    from vitcnn_amd._lib import lib
    return lib().raw


def test_conv_option_builds_the_same_model():
    from vitcnn_amd.mhst import MHST
    direct = build("mhst_b")
    assert direct.conv == "direct"
    torch.manual_seed(0)
    mfma = MHST(**CASES["mhst_b"], **REGISTRY, conv="mfma")
    assert mfma.conv == "mfma"
    a, b = direct.state_dict(), mfma.state_dict()
    assert list(a) == list(b) and len(a) == 150
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert mfma.set_conv("direct") is mfma and mfma.conv == "direct"
    assert mfma.set_conv("mfma").conv == "mfma"


def test_conv_option_rejects_unknown_modes():
    from vitcnn_amd.mhst import MHST
    with pytest.raises(ValueError):
        MHST(**CASES["mhst_b"], **REGISTRY, conv="im2col")
    m = build("mhst_b")
    with pytest.raises(ValueError):
        m.set_conv("im2col")
    assert m.conv == "direct"
    with pytest.raises(TypeError):     # keyword only: the positional signature is the reference's
        MHST(*([11, 2, 8, 64, 12, 64, 1, 4, 8] + [None] * 13 + ["mfma"]))


def test_get_model_passes_conv_through():
    from vitcnn_amd import model_utils as mu
    args = dict(n_classes=16, n_bands=(144, 1), ignored_labels=[0], dataset="Houston2013", device=torch.device("cpu"))
    torch.manual_seed(0)
    model, _, _, kw = mu.get_model("MHST", **args, conv="mfma")
    assert model.conv == "mfma" and kw["conv"] == "mfma"
    torch.manual_seed(0)
    ref, _, _, kw0 = mu.get_model("MHST", **args)
    assert ref.conv == "direct" and kw0["conv"] == "direct"
    a, b = ref.state_dict(), model.state_dict()
    assert list(a) == list(b) and len(a) == 338
    assert all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(ValueError):
        mu.get_model("MHST", **args, conv="im2col")


@pytest.mark.parametrize("D", DEPTHS)
def test_pconv_ok_accepts_the_hsi_sites(D):
    ok, ws = raw()["vc_mhst_pconv_ok"], raw()["vc_mhst_pconv_ws_floats"]
    for C, O, G, KS, ldx, ldy in HSI:
        assert ok(D, C, O, G, KS, ldx, ldy) == 1, (D, G, KS)
        assert ok(D, C, O, G, KS, 20, 64) == 1       # rows longer than natural that keep 16-byte alignment
        assert ws(64, D, C, O, G, KS) > 0


def test_pconv_ok_accepts_the_lidar_and_classifier_sites():
    ok, ws = raw()["vc_mhst_pconv_ok"], raw()["vc_mhst_pconv_ws_floats"]
    for C, O, G, KS, ldx, ldy in LIDAR + CLASSIFIER:
        assert ok(1, C, O, G, KS, ldx, ldy) == 1, (C, KS)
        assert ws(64, 1, C, O, G, KS) > 0


@pytest.mark.parametrize("what,args", [
    ("even KS", (3, 16, 16, 1, 4, 16, 64)),
    ("KS = 11", (3, 16, 16, 1, 11, 16, 64)),
    ("KS = 1", (3, 16, 16, 1, 1, 16, 64)),
    ("O % G", (3, 16, 12, 8, 3, 16, 64)),
    ("C % G", (3, 12, 16, 8, 3, 12, 64)),
    ("ldx = 18: rows off 16 bytes", (3, 16, 16, 1, 3, 18, 64)),
    ("ldx = 17", (3, 16, 16, 1, 3, 17, 64)),
    ("ldy = 66", (3, 16, 16, 1, 3, 16, 66)),
    ("ldx < C", (3, 16, 16, 1, 3, 12, 64)),
    ("ldy < O", (3, 16, 16, 1, 3, 16, 12)),
    ("D = 0", (0, 16, 16, 1, 3, 16, 64)),
    ("LiDAR conv1: 1 input channel", (1, 1, 8, 1, 3, 4, 32)),
    ("LiDAR conv1: 3 input channels", (1, 3, 8, 1, 9, 4, 32)),
    ("LiDAR conv1: 2 input channels in rows of 4", (1, 2, 8, 1, 5, 4, 32)),
    ("one channel per group", (3, 16, 16, 16, 3, 16, 64)),
])
def test_pconv_ok_refuses(what, args):
    assert raw()["vc_mhst_pconv_ok"](*args) == 0, what


def test_pconv_ws_floats_refuses_what_ok_refuses():
    ws = raw()["vc_mhst_pconv_ws_floats"]
    assert ws(0, 3, 16, 16, 1, 3) == -1
    assert ws(2, 3, 16, 16, 1, 4) == -1
    assert ws(2, 1, 3, 8, 1, 9) == -1


P = 4096   # stands for a 16-byte aligned device address: a refused call returns before anything reads it


def _calls(B, D, C, O, G, KS, ldx, ldy, ws_floats, x=P, y=P, w=P, ws=P):
    """the three entry points on one shape; dgrad's x side is dx, its y side dy"""
    r = raw()
    return (r["vc_mhst_pconv_fwd"](B, D, C, O, G, KS, x, ldx, w, None, y, ldy, ws, ws_floats, None),
            r["vc_mhst_pconv_dgrad"](B, D, C, O, G, KS, y, ldy, w, x, ldx, 0.0, ws, ws_floats, None),
            r["vc_mhst_pconv_wgrad"](B, D, C, O, G, KS, x, ldx, y, ldy, w, None, ws, ws_floats, None))


def test_pconv_entry_points_refuse_on_the_host():
    n = raw()["vc_mhst_pconv_ws_floats"](2, 3, 16, 16, 2, 5)
    assert n > 0
    assert _calls(2, 3, 16, 16, 2, 5, 16, 64, n - 1) == (1, 1, 1)          # the workspace one float short
    assert _calls(2, 3, 16, 16, 2, 4, 16, 64, 1 << 30) == (1, 1, 1)        # a shape _ok refuses: even KS
    assert _calls(2, 3, 16, 16, 2, 5, 18, 64, 1 << 30) == (1, 1, 1)        # rows off 16 bytes
    assert _calls(2, 3, 12, 16, 8, 3, 12, 64, 1 << 30) == (1, 1, 1)        # C % G
    assert _calls(0, 3, 16, 16, 2, 5, 16, 64, n) == (1, 1, 1)              # an empty batch
    assert _calls(2, 3, 16, 16, 2, 5, 16, 64, n, x=None) == (1, 1, 1)      # null pointers
    assert _calls(2, 3, 16, 16, 2, 5, 16, 64, n, ws=None) == (1, 1, 1)
    assert _calls(2, 3, 16, 16, 2, 5, 16, 64, n, w=None) == (1, 1, 1)
    assert _calls(2, 3, 16, 16, 2, 5, 16, 64, n, x=P + 4) == (1, 1, 1)     # the x side off 16 bytes
    assert _calls(2, 3, 16, 16, 2, 5, 16, 64, n, y=P + 8) == (1, 1, 1)     # a column offset of 2 floats
