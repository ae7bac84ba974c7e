"""Guards that need no GPU: every entry point of include/vitcnn.h is named by some test, and the S2EFT /
FusAtNet / glue entry points, LayerNorm, vc_gemm and the Mamba scan refuse invalid arguments on the host, before
any launch."""
import glob
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Entry points no test has to name: measurement hooks only, one line of reason each, two entries at the most.
UNTESTED_ALLOWED = {
    "vc_gemm_tune": "forces a GEMM plan in the probe library only; the product library accepts the automatic one",
}


def test_every_entry_point_is_named_by_a_test():
    from vitcnn_amd._lib import parse_header
    assert len(UNTESTED_ALLOWED) <= 2
    names = set(parse_header())
    assert len(names) >= 100 and set(UNTESTED_ALLOWED) <= names
    text = ""
    for path in sorted(glob.glob(os.path.join(REPO, "tests", "test_*.py"))):
        if os.path.abspath(path) != os.path.abspath(__file__):    # the rejection cases below are no parity tests
            text += open(path).read()
    used = set(re.findall(r"\bvc_\w+\b", text))
    missing = sorted(names - used - set(UNTESTED_ALLOWED))
    assert not missing, f"entry points no tests/test_*.py calls: {missing}"


def _raw():
    from vitcnn_amd._lib import lib
    return lib().raw


REJECTED = [
    ("attention T = 0", "vc_s2eft_attn_fwd", (1, 0, 4, None, 0.25, None, None, None)),
    ("attention T = 257", "vc_s2eft_attn_fwd", (1, 257, 4, None, 0.25, None, None, None)),
    ("attention backward T = 0", "vc_s2eft_attn_bwd", (1, 0, 4, None, None, None, None, 0.25, None, None)),
    ("attention backward T = 257", "vc_s2eft_attn_bwd", (1, 257, 4, None, None, None, None, 0.25, None, None)),
    ("dropout p = 1", "vc_dropout_fwd", (16, None, None, None, None, 1.0, 0, None)),
    ("dropout p < 0", "vc_dropout_fwd", (16, None, None, None, None, -0.25, 0, None)),
    ("dropout backward p = 1", "vc_dropout_bwd", (16, None, None, 1.0, None, None)),
    ("dropout backward p < 0", "vc_dropout_bwd", (16, None, None, -0.25, None, None)),
    ("cat2 exchange with C1 != C2", "vc_cat2_fwd", (4, 8, 6, None, 8, None, 6, 1, None, None)),
    ("cat2 backward exchange with C1 != C2", "vc_cat2_bwd", (4, 8, 6, None, 1, None, 8, 0.0, None, 6, 0.0, None)),
    ("im2col pad = 2", "vc_im2col3x3_pad", (1, 5, 5, 4, 2, None, 4, None, None)),
    ("im2col ldx < C", "vc_im2col3x3_pad", (1, 5, 5, 4, 1, None, 3, None, None)),
    ("im2col H = 2 without padding", "vc_im2col3x3_pad", (1, 2, 5, 4, 0, None, 4, None, None)),
    ("adamw params not 16-B aligned", "vc_adamw", (8, 4, None, None, None, None, None, None)),
    ("adamw grads not 16-B aligned", "vc_adamw", (8, None, 4, None, None, None, None, None)),
    ("gate N = 4097", "vc_s2eft_gate_fwd", (1, 4097, 8, None, None, None, 0.4, None, None, None)),
    ("layernorm C = 0", "vc_layernorm_fwd", (4, 0, None, 0, None, None, 1e-6, None, 0, None, None, None)),
    ("layernorm C = 513", "vc_layernorm_fwd", (4, 513, None, 513, None, None, 1e-6, None, 513, None, None, None)),
    ("gemm batch = 0", "vc_gemm", (0, 0, 4, 4, 4, 1.0, None, 4, 0, None, 4, 0, 0.0, None, 4, 0, 0, None, None, 0, 0, 0,
                                   None, None, 0, None)),
    ("gemm bias_grad with batch = 2", "vc_gemm", (1, 0, 4, 4, 4, 1.0, None, 4, 16, None, 4, 16, 0.0, None, 4, 16, 2, None,
                                                  None, 0, 0, 0, 4, None, 0, None)),
    ("scan D = 129", "vc_mamba_scan_fwd", (1, 4, 129, 9, 1, None, None, None, None, None, None, None, None, None, None)),
    ("scan R = 65", "vc_mamba_scan_fwd", (1, 4, 72, 65, 1, None, None, None, None, None, None, None, None, None, None)),
]


def test_scan_ckpt_floats_rejects_an_empty_batch():
    assert _raw()["vc_mamba_scan_ckpt_floats"](0, 81, 72, 10) == -1


@pytest.mark.parametrize("what,name,args", REJECTED, ids=[r[0] for r in REJECTED])
def test_host_side_rejections(what, name, args):
    """VC_REQUIRE returns 1 (hipErrorInvalidValue) before any launch: null pointers are never touched"""
    assert _raw()[name](*args) == 1, what
