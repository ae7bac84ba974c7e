"""FusAtNet's precision switch without a GPU: `get_model("FusAtNet", precision=...)` and
`FusAtNet.set_precision` carry the precision, the state_dict does not depend on it, the four flagged tap-major conv
entry points (vc_conv3x3_tap_fwd_ex, vc_conv3x3_tap_wgrad_ex, vc_conv3x3_tap_wgrad_oihw_ex, vc_conv3x3_tap_dgrad_ex)
refuse unknown flag bits and bad geometry on the host, and the bf16-operand CPU oracle of the GPU tests
(tests/fusat_bf16_oracle.py) with its rounding off is the pinned oracle: it reproduces the reference's golden logits.
"""
import os

import numpy as np
import pytest
import torch

import fusat_bf16_oracle as R

HERE = os.path.dirname(os.path.abspath(__file__))
KW = dict(n_classes=16, n_bands=(144, 1), ignored_labels=[0], dataset="Houston2013", device=torch.device("cpu"))


def _get(**extra):
    from vitcnn_amd.model_utils import get_model
    return get_model("FusAtNet", **dict(KW, **extra))


def test_get_model_carries_the_precision():
    model, _, _, kw = _get(precision="bf16")
    assert model.precision == "bf16" and kw["precision"] == "bf16"
    model, _, _, kw = _get()
    assert model.precision == "fp32" and kw["precision"] == "fp32"


def test_unknown_precision_raises():
    from vitcnn_amd.fusatnet import FusAtNet
    with pytest.raises(ValueError):
        _get(precision="fp16")
    with pytest.raises(ValueError):
        FusAtNet(144, 1, 16, precision="fp16")
    m = FusAtNet(144, 1, 16)
    with pytest.raises(ValueError):
        m.set_precision("fp16")
    assert m.precision == "fp32"


def test_set_precision_round_trips():
    from vitcnn_amd.fusatnet import FusAtNet
    m = FusAtNet(144, 1, 16)
    assert m.precision == "fp32"
    assert m.set_precision("bf16") is m and m.precision == "bf16"
    assert m.set_precision("fp32") is m and m.precision == "fp32"


def test_state_dict_is_independent_of_precision():
    from vitcnn_amd.fusatnet import FusAtNet
    torch.manual_seed(0)
    a = FusAtNet(144, 1, 16)
    torch.manual_seed(0)
    b = FusAtNet(144, 1, 16, precision="bf16")
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    b.set_precision("fp32")
    assert list(b.state_dict()) == list(sa)
    a.set_precision("bf16").load_state_dict(sb)
    assert a.precision == "bf16"


# (B, H, W, C, O, pad) then the direction's operands; P: a non-null address no refused call ever touches
P = 4096
_GEO = (1, 5, 5, 4, 4)


def _fwd(pad=0, ldy=4, flags=0):
    return _GEO + (pad, P, 4, P, None, P, ldy, None, 0, flags, None)


def _wgrad(pad=0, lddy=4, flags=0):
    return _GEO + (pad, P, 4, P, lddy, P, None, 0, flags, None)


def _wgrad_oihw(pad=0, lddy=4, flags=0):
    return _GEO + (pad, P, 4, P, lddy, P, None, None, 0, flags, None)


def _dgrad(pad=0, lddy=4, flags=0):
    return _GEO + (pad, P, lddy, P, 0.0, P, 4, None, 0, flags, None)


REJECTED = []
for _name, _mk, _ld in (("vc_conv3x3_tap_fwd_ex", _fwd, "ldy"), ("vc_conv3x3_tap_wgrad_ex", _wgrad, "lddy"),
                        ("vc_conv3x3_tap_wgrad_oihw_ex", _wgrad_oihw, "lddy"),
                        ("vc_conv3x3_tap_dgrad_ex", _dgrad, "lddy")):
    REJECTED += [(f"{_name} flags = 4", _name, _mk(flags=4)),
                 (f"{_name} flags = 6", _name, _mk(flags=6)),
                 (f"{_name} pad = 2", _name, _mk(pad=2)),
                 (f"{_name} pad = 2, bf16", _name, _mk(pad=2, flags=2)),
                 (f"{_name} {_ld} < O", _name, _mk(**{_ld: 3})),
                 (f"{_name} {_ld} < O, bf16", _name, _mk(**{_ld: 3, "flags": 2}))]


@pytest.mark.parametrize("what,name,args", REJECTED, ids=[r[0] for r in REJECTED])
def test_ex_host_side_rejections(what, name, args):
    """VC_REQUIRE returns 1 before any launch; every other argument of the call is valid, so the refusal is the
    named one (the pointers are never touched)"""
    from vitcnn_amd._lib import lib
    assert lib().raw[name](*args) == 1, what


def test_oracle_without_rounding_is_the_pinned_oracle():
    """the wrapper with the conv substituted but the rounding off reproduces the reference's train-mode logits to the
    bound of test_fusat_state_dict_and_oracle_match_reference -- and with the rounding on it does not"""
    from vitcnn_amd.fusatnet import FusAtNet
    z = np.load(os.path.join(HERE, "golden", "fusat_b4.npz"))
    torch.manual_seed(0)
    m = FusAtNet(144, 1, 16)
    x1, x2 = torch.from_numpy(z["x1"]), torch.from_numpy(z["x2"])
    want = torch.from_numpy(z["logits_train"])

    def rel(a, b):
        return float((a - b).norm() / b.norm())

    with torch.no_grad():
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        plain = R.forward(sd, x1, x2, train=True, rounding=False)
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        rounded = R.forward(sd, x1, x2, train=True, rounding=True)
    assert rel(plain, want) < 1e-5
    assert rel(rounded, want) > 1e-3
    from oracle import fusat_oracle as O
    import torch.nn.functional as F
    assert O.F is F   # the substitution is undone


def test_rounded_conv_gradients_are_those_of_rounded_operands():
    """RoundedConv3x3's backward: dw and dx are the float64 conv gradients of rounded x, w and rounded dy; db is the
    sum of the unrounded dy"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 6, 6, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(7, 5, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(7, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(2, 7, 6, 6, generator=g, dtype=torch.float64)
    R.RoundedConv3x3.apply(x, w, b, 1).backward(dy)
    xr = R.rne_bf16(x.detach()).requires_grad_(True)
    wr = R.rne_bf16(w.detach()).requires_grad_(True)
    y = F.conv2d(xr, wr, b.detach(), padding=1)
    y.backward(R.rne_bf16(dy))
    assert torch.allclose(x.grad, xr.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(w.grad, wr.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(b.grad, dy.sum(dim=(0, 2, 3)), rtol=1e-12, atol=1e-12)
    assert not torch.equal(R.rne_bf16(dy), dy)
