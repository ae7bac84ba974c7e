"""MHST's third conv mode and the vc_mhst_conv1_* / vc_mhst_sconv_* families without a GPU: the "mfma_all" model is the
"direct" model (same state_dict keys and initial values), get_model passes the option through, a bad mode raises and
leaves the mode as it was; the workspace queries answer on the host; every launching entry point returns 1 on the host,
before any launch, for an empty batch or depth, a bad leading dimension, a null or misaligned operand, biases partly null
and a short workspace."""
import pytest
import torch

from mhst_cases import CASES, REGISTRY, build


def raw():
    from vitcnn_amd._lib import lib
    return lib().raw


def test_mfma_all_builds_the_same_model():
    from vitcnn_amd.mhst import CONV_MODES, MHST
    assert CONV_MODES == ("direct", "mfma", "mfma_all")
    direct = build("mhst_b")
    torch.manual_seed(0)
    m = MHST(**CASES["mhst_b"], **REGISTRY, conv="mfma_all")
    assert m.conv == "mfma_all"
    a, b = direct.state_dict(), m.state_dict()
    assert list(a) == list(b) and len(a) == 150
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert direct.set_conv("mfma_all") is direct and direct.conv == "mfma_all"
    assert direct.set_conv("mfma").conv == "mfma" and direct.set_conv("direct").conv == "direct"


def test_an_unknown_mode_still_raises_and_leaves_the_mode():
    from vitcnn_amd.mhst import MHST
    m = build("mhst_b").set_conv("mfma_all")
    for bad in ("mfma_everything", "MFMA_ALL", "", None):
        with pytest.raises(ValueError):
            m.set_conv(bad)
        assert m.conv == "mfma_all"
    with pytest.raises(ValueError):
        MHST(**CASES["mhst_b"], **REGISTRY, conv="all")


def test_get_model_passes_mfma_all_through():
    from vitcnn_amd import model_utils as mu
    args = dict(n_classes=16, n_bands=(144, 1), ignored_labels=[0], dataset="Houston2013", device=torch.device("cpu"))
    torch.manual_seed(0)
    model, _, _, kw = mu.get_model("MHST", **args, conv="mfma_all")
    assert model.conv == "mfma_all" and kw["conv"] == "mfma_all"
    torch.manual_seed(0)
    ref, _, _, _ = mu.get_model("MHST", **args)
    a, b = ref.state_dict(), model.state_dict()
    assert list(a) == list(b) and len(a) == 338
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_the_workspace_queries():
    c1, sc = raw()["vc_mhst_conv1_ws_floats"], raw()["vc_mhst_sconv_ws_floats"]
    for B, l1 in ((1, 1), (64, 144), (4, 512)):
        assert c1(B, l1) > 0, (B, l1)
    for B, D in ((1, 1), (64, 48)):
        assert sc(B, D) > 0, (B, D)
    assert c1(0, 144) < 0 and c1(4, 0) < 0
    assert sc(0, 48) < 0 and sc(4, 0) < 0
    assert c1(3, 30) >= c1(1, 30) and sc(3, 10) >= sc(1, 10)


P = 4096   # stands for a 16-byte aligned device address: a refused call returns before anything reads it


def _conv1(B=2, l1=30, x=P, w=P, bias=P, y=P, ldy=16, dw=P, ws=P, short=0):
    r = raw()
    n = max(r["vc_mhst_conv1_ws_floats"](max(B, 1), max(l1, 1)), 1) - short
    # never a call that would pass the checks: a refused call returns before anything is launched or read
    return (r["vc_mhst_conv1_fwd"](B, l1, x, w, bias, y, ldy, ws, n, None) if dw is not None else 1,
            r["vc_mhst_conv1_wgrad"](B, l1, x, y, ldy, dw, None, ws, n, None) if w is not None else 1)


def test_conv1_entry_points_refuse_on_the_host():
    assert _conv1(B=0) == (1, 1)
    assert _conv1(l1=0) == (1, 1)
    assert _conv1(ldy=12) == (1, 1)          # below 16
    assert _conv1(ldy=18) == (1, 1)          # rows off 16 bytes
    assert _conv1(x=None) == (1, 1)
    assert _conv1(y=None) == (1, 1)
    assert _conv1(ws=None) == (1, 1)
    assert _conv1(w=None) == (1, 1)          # the forward alone: the weight gradient takes no weight
    assert _conv1(dw=None) == (1, 1)         # the weight gradient alone
    assert _conv1(x=P + 4) == (1, 1)
    assert _conv1(y=P + 8) == (1, 1)
    assert _conv1(ws=P + 4) == (1, 1)
    assert _conv1(short=1) == (1, 1)         # the workspace one float short


def _sconv(B=2, D=10, x=P, ldx=16, y=P, ldy=16, w=(P, P, P, P), b=(P, P, P, P), ws=P, short=0):
    """the three entry points; dgrad's x side is dx, its y side dy; the weight gradient's outputs stand where w and b do"""
    r = raw()
    n = max(r["vc_mhst_sconv_ws_floats"](max(B, 1), max(D, 1)), 1) - short
    # never a call that would pass the checks: the data gradient takes no bias, so a bias case leaves it out
    return (r["vc_mhst_sconv_fwd"](B, D, x, ldx, *w, *b, y, ldy, ws, n, None),
            r["vc_mhst_sconv_dgrad"](B, D, y, ldy, *w, x, ldx, 0.0, ws, n, None) if b == (P, P, P, P) else 1,
            r["vc_mhst_sconv_wgrad"](B, D, x, ldx, y, ldy, *w, *b, ws, n, None))


def test_sconv_entry_points_refuse_on_the_host():
    assert _sconv(B=0) == (1, 1, 1)
    assert _sconv(D=0) == (1, 1, 1)
    assert _sconv(ldx=12) == (1, 1, 1)
    assert _sconv(ldx=18) == (1, 1, 1)
    assert _sconv(ldy=8) == (1, 1, 1)
    assert _sconv(ldy=22) == (1, 1, 1)
    assert _sconv(x=None) == (1, 1, 1)
    assert _sconv(y=None) == (1, 1, 1)
    assert _sconv(ws=None) == (1, 1, 1)
    assert _sconv(w=(P, P, None, P)) == (1, 1, 1)
    assert _sconv(x=P + 4) == (1, 1, 1)
    assert _sconv(y=P + 8) == (1, 1, 1)
    assert _sconv(ws=P + 12) == (1, 1, 1)
    assert _sconv(short=1) == (1, 1, 1)
    # biases partly null: the forward's biases and the weight gradient's bias gradients (dgrad takes none)
    fwd, _, wgrad = _sconv(b=(P, None, P, P))
    assert (fwd, wgrad) == (1, 1)
    fwd, _, wgrad = _sconv(b=(None, None, None, P))
    assert (fwd, wgrad) == (1, 1)
