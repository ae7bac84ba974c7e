"""FusAtNet's `precision="bf16_store"` without a GPU: the constructor, `set_precision` and
`get_model("FusAtNet", ...)` accept the value, ViT-CNN keeps refusing it and `model.PRECISIONS` is what it was, the
header declares the new entry points, and those refuse a leading dimension that is no multiple of 8, a base that is not
16-B aligned and a null operand with status 1 on the host, before any HIP call."""
import pytest
import torch

KW = dict(n_classes=16, n_bands=(144, 1), ignored_labels=[0], dataset="Houston2013", device=torch.device("cpu"))
NEW = ("vc_cast_bf16_2d", "vc_conv3x3_pack_bf16_many", "vc_conv3x3_tap_fwd_h", "vc_conv3x3_tap_wgrad_oihw_h",
       "vc_conv3x3_tap_dgrad_h", "vc_bn_forward_ex_h", "vc_bn_bwd_relu_ex_h")


def test_fusatnet_accepts_bf16_store():
    from vitcnn_amd.fusatnet import FusAtNet
    from vitcnn_amd.model_utils import get_model
    m = FusAtNet(144, 1, 16, precision="bf16_store")
    assert m.precision == "bf16_store"
    assert m.set_precision("bf16") is m and m.precision == "bf16"
    assert m.set_precision("bf16_store") is m and m.precision == "bf16_store"
    with pytest.raises(ValueError):
        m.set_precision("bf16_stored")
    assert m.precision == "bf16_store"
    model, _, _, kw = get_model("FusAtNet", **dict(KW, precision="bf16_store"))
    assert model.precision == "bf16_store" and kw["precision"] == "bf16_store"


def test_state_dict_is_independent_of_bf16_store():
    from vitcnn_amd.fusatnet import FusAtNet
    torch.manual_seed(0)
    a = FusAtNet(144, 1, 16)
    torch.manual_seed(0)
    b = FusAtNet(144, 1, 16, precision="bf16_store")
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_vitcnn_refuses_bf16_store():
    from vitcnn_amd import model
    assert model.PRECISIONS == ("fp32", "bf16")
    with pytest.raises(ValueError):
        model.Multimodality_Mamba(precision="bf16_store")
    from vitcnn_amd.model_utils import get_model
    with pytest.raises(ValueError):
        get_model("Multimodality_Mamba", **dict(KW, precision="bf16_store"))


def test_launch_offers_the_choice():
    from vitcnn_amd import launch
    assert any("'bf16_store'" in repl for _, repl in launch._EDITS)


def test_header_declares_the_entry_points():
    from vitcnn_amd._lib import parse_header
    sigs = parse_header()
    for name in NEW:
        assert name in sigs, name
    assert len(sigs["vc_conv3x3_tap_fwd_h"]) == len(sigs["vc_conv3x3_tap_fwd"])
    assert len(sigs["vc_conv3x3_tap_wgrad_oihw_h"]) == len(sigs["vc_conv3x3_tap_wgrad_oihw"]) - 1   # no db
    assert len(sigs["vc_bn_forward_ex_h"]) == len(sigs["vc_bn_forward_ex"]) + 2
    assert len(sigs["vc_bn_bwd_relu_ex_h"]) == len(sigs["vc_bn_bwd_relu_ex"]) + 2


# P: a non-null 16-B aligned address no refused call ever touches; (B, H, W, C, O) with C = O = 16
P = 4096
_GEO = (1, 5, 5, 16, 16)


def _fwd(x=P, ldx=16, wt=P):
    return _GEO + (1, x, ldx, wt, None, P, 16, None, 0, None)


def _wgrad(x=P, ldx=16, dy=P, lddy=16):
    return _GEO + (1, x, ldx, dy, lddy, P, None, 0, None)


def _dgrad(dy=P, lddy=16, wt=P):
    return _GEO + (1, dy, lddy, wt, 0.0, P, 16, None, 0, None)


_BN_F = (1, 8, 16, P, 16, 1e-5, 0.1, P, P, P, P, P, P, 1, P, 16)
_BN_B = (1, 8, 16, P, 16, P, 16, P, P, P, P, P, 16, 0.0)
_BN_T = (P, 1 << 16, None, 0, None)

REJECTED = [
    ("fwd ldx16 % 8", "vc_conv3x3_tap_fwd_h", _fwd(ldx=20)),
    ("fwd ldx16 < C", "vc_conv3x3_tap_fwd_h", _fwd(ldx=8)),
    ("fwd x16 misaligned", "vc_conv3x3_tap_fwd_h", _fwd(x=P + 2)),
    ("fwd wt16 misaligned", "vc_conv3x3_tap_fwd_h", _fwd(wt=P + 8)),
    ("fwd x16 null", "vc_conv3x3_tap_fwd_h", _fwd(x=None)),
    ("fwd wt16 null", "vc_conv3x3_tap_fwd_h", _fwd(wt=None)),
    ("wgrad ldx16 % 8", "vc_conv3x3_tap_wgrad_oihw_h", _wgrad(ldx=20)),
    ("wgrad lddy16 % 8", "vc_conv3x3_tap_wgrad_oihw_h", _wgrad(lddy=20)),
    ("wgrad x16 misaligned", "vc_conv3x3_tap_wgrad_oihw_h", _wgrad(x=P + 4)),
    ("wgrad dy16 misaligned", "vc_conv3x3_tap_wgrad_oihw_h", _wgrad(dy=P + 2)),
    ("wgrad x16 null", "vc_conv3x3_tap_wgrad_oihw_h", _wgrad(x=None)),
    ("wgrad dy16 null", "vc_conv3x3_tap_wgrad_oihw_h", _wgrad(dy=None)),
    ("dgrad lddy16 % 8", "vc_conv3x3_tap_dgrad_h", _dgrad(lddy=20)),
    ("dgrad dy16 misaligned", "vc_conv3x3_tap_dgrad_h", _dgrad(dy=P + 2)),
    ("dgrad wt16 misaligned", "vc_conv3x3_tap_dgrad_h", _dgrad(wt=P + 8)),
    ("dgrad dy16 null", "vc_conv3x3_tap_dgrad_h", _dgrad(dy=None)),
    ("dgrad wt16 null", "vc_conv3x3_tap_dgrad_h", _dgrad(wt=None)),
    ("cast ldd % 8", "vc_cast_bf16_2d", (4, 5, P, 5, P, 7, None)),
    ("cast ldd < C", "vc_cast_bf16_2d", (4, 9, P, 9, P, 8, None)),
    ("cast dst misaligned", "vc_cast_bf16_2d", (4, 5, P, 5, P + 2, 8, None)),
    ("cast dst null", "vc_cast_bf16_2d", (4, 5, P, 5, None, 8, None)),
    ("cast src null", "vc_cast_bf16_2d", (4, 5, None, 5, P, 8, None)),
    ("bn forward ld16 % 8", "vc_bn_forward_ex_h", _BN_F + (P, 20) + _BN_T),
    ("bn forward y16 misaligned", "vc_bn_forward_ex_h", _BN_F + (P + 2, 16) + _BN_T),
    ("bn backward ld16 % 8", "vc_bn_bwd_relu_ex_h", _BN_B + (P, 20, P, P, 0.0) + _BN_T),
    ("bn backward dx16 misaligned", "vc_bn_bwd_relu_ex_h", _BN_B + (P + 2, 16, P, P, 0.0) + _BN_T),
]


@pytest.mark.parametrize("what,name,args", REJECTED, ids=[r[0] for r in REJECTED])
def test_host_side_refusals(what, name, args):
    """VC_REQUIRE returns 1 before any HIP call; every other argument of the call is valid, so the refusal is the
    named one (the pointers are never touched)"""
    from vitcnn_amd._lib import lib
    assert lib().raw[name](*args) == 1, what


def test_pack_refuses_a_misaligned_arena():
    import ctypes
    from vitcnn_amd._lib import lib
    shapes = (ctypes.c_int * 2)(16, 16)
    src = (ctypes.c_void_p * 1)(P)
    for bad in (P + 2, None):
        dst = (ctypes.c_void_p * 1)(bad)
        assert lib().raw["vc_conv3x3_pack_bf16_many"](1, ctypes.addressof(shapes), ctypes.addressof(src),
                                                      ctypes.addressof(dst), None) == 1
