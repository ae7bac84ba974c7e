"""Guards that need no GPU: every entry point of include/vitcnn.h is named by some test, and the S2EFT /
FusAtNet / glue entry points, LayerNorm, vc_gemm, the Mamba scan, the 3x3 convolutions, the max pool, the non-local
attention, the row chains and the TokenLearner refuse invalid arguments on the host, before any launch."""
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
    # the spatial half (conv_gemm / conv_tap / conv / attention / rowchain / tokenlearner)
    ("conv3x3 pad = 2", "vc_conv3x3_fwd", (1, 5, 5, 4, 4, 2, None, 4, None, None, None, None, None, None, 1, None, 4,
                                           None, 0, None)),
    ("conv3x3 ldy < O", "vc_conv3x3_fwd", (1, 5, 5, 4, 4, 0, None, 4, None, None, None, None, None, None, 1, None, 3,
                                           None, 0, None)),
    ("tap dgrad lddx < C", "vc_conv3x3_tap_dgrad", (1, 5, 5, 4, 4, 0, None, 4, None, 0.0, None, 3, None, 0, None)),
    ("maxpool ldx < C", "vc_maxpool2_fwd", (1, 4, 4, 8, None, 7, None, None, None)),
    ("nonlocal P = 17", "vc_nonlocal_attn_fwd", (1, 9, 17, 8, None, None, None, None, None)),
    ("nonlocal P = 5 at Ci = 6 (no wave-per-row kernel for 5 keys)", "vc_nonlocal_attn_fwd",
     (1, 9, 5, 6, None, None, None, None, None)),
    ("nonlocal P = 5 with theta off 16 B", "vc_nonlocal_attn_fwd", (1, 9, 5, 8, 4, None, None, None, None)),
    ("nonlocal backward P = 5 at Ci = 6", "vc_nonlocal_attn_bwd", (1, 9, 5, 6, None, None, None, None, None, None, None)),
    ("nonlocal pool (Hs / 2)^2 != P", "vc_nonlocal_attn_pool_fwd", (1, 36, 4, 8, 6, None, None, 16, None, None, None,
                                                                   None, None)),
    ("nonlocal pool ldpg < 2 Ci", "vc_nonlocal_attn_pool_fwd", (1, 16, 4, 8, 4, None, None, 15, None, None, None, None,
                                                                None)),
    ("rowchain front E = 260", "vc_rowchain_front", (16, 144, 260, 144, None, None, None, 9, None, None, None, 1e-6, None,
                                                     None, None, None, None, None)),
    ("rowchain front K0 = 6", "vc_rowchain_front", (16, 6, 144, 144, None, None, None, 9, None, None, None, 1e-6, None,
                                                    None, None, None, None, None)),
    ("rowchain back_bwd dcd at address 4", "vc_rowchain_back_bwd", (16, 144, 144, 72, 4, None, None, None, None, None,
                                                                    None, None, None, None, None, None, None, None)),
    ("rowchain back_bwd Cout = 6", "vc_rowchain_back_bwd", (16, 6, 144, 72, None, None, None, None, None, None, None,
                                                            None, None, None, None, None, None, None)),
    ("rowchain front_bwd K0 = 6", "vc_rowchain_front_bwd", (16, 6, 144, 3, None, None, None, None, None, None, None, None,
                                                            None, None, None, 0.0, None, None)),
    ("rowchain front_bwd E = 6", "vc_rowchain_front_bwd", (16, 144, 6, 3, None, None, None, None, None, None, None, None,
                                                           None, None, None, 0.0, None, None)),
    ("tl_bwd C = 513", "vc_tl_bwd", (1, 2, 49, 513, 25, None, 513, None, None, None, None, None, None, None, None, None,
                                     513, None, None)),
    # (401 pixels with 324 tokens are accepted: the token and pixel chunks shrink until their LDS plans fit)
    ("tl_check 30 x 30 pixels: no token chunk fits the LDS", "vc_tl_check", (900, 256, 324)),
    ("tl_check C = 513", "vc_tl_check", (400, 513, 324)),
]


def test_scan_ckpt_floats_rejects_an_empty_batch():
    assert _raw()["vc_mamba_scan_ckpt_floats"](0, 81, 72, 10) == -1


@pytest.mark.parametrize("what,name,args", REJECTED, ids=[r[0] for r in REJECTED])
def test_host_side_rejections(what, name, args):
    """VC_REQUIRE returns 1 (hipErrorInvalidValue) before any launch: null pointers are never touched"""
    assert _raw()[name](*args) == 1, what
