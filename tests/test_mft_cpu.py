"""Host-side rejections of the MFT entry points (csrc/mft.hip): VC_REQUIRE returns 1 (hipErrorInvalidValue) before
any launch, so null pointers are never touched and no GPU is needed (the style of test_coverage_cpu.py's table)."""
import pytest


def _raw():
    from vitcnn_amd._lib import lib
    return lib().raw


N = None
REJECTED = [
    ("conv3d NC - 8 < 1", "vc_mft_conv3d_fwd", (2, 8, 11, N, N, N, N, 0, N)),
    ("conv3d P = 4, below the minimum", "vc_mft_conv3d_fwd", (2, 30, 4, N, N, N, N, 176, N)),
    ("conv3d P = 29, above the LDS plan", "vc_mft_conv3d_fwd", (2, 30, 29, N, N, N, N, 176, N)),
    ("conv3d ldy < 8 D", "vc_mft_conv3d_fwd", (2, 30, 11, N, N, N, N, 172, N)),
    ("conv3d ldy not a multiple of 4", "vc_mft_conv3d_fwd", (2, 30, 11, N, N, N, N, 177, N)),
    ("conv3d wgrad NC - 8 < 1", "vc_mft_conv3d_wgrad", (2, 8, 11, N, N, 0, N, N, N, 0, N)),
    ("conv3d wgrad P = 4", "vc_mft_conv3d_wgrad", (2, 30, 4, N, N, 176, N, N, N, 0, N)),
    ("conv3d wgrad without a workspace", "vc_mft_conv3d_wgrad", (2, 30, 11, N, N, 176, N, N, N, 0, N)),
    ("hetconv pack C % g != 0", "vc_mft_hetconv_pack", (64, 24, 16, N, N, N, N, N, N, N)),
    ("hetconv pack C % 8 != 0", "vc_mft_hetconv_pack", (64, 12, 4, N, N, N, N, N, N, N)),
    ("hetconv unpack O % g != 0", "vc_mft_hetconv_unpack", (60, 32, 16, N, N, N, N)),
    ("tokpool L = 5", "vc_mft_tokpool_fwd", (2, 121, 5, N, 64, N, N, N, N, N, N, 64, 320, N)),
    ("tokpool HW = 1025", "vc_mft_tokpool_fwd", (2, 1025, 4, N, 64, N, N, N, N, N, N, 64, 320, N)),
    ("tokpool ldx < 64", "vc_mft_tokpool_fwd", (2, 121, 4, N, 60, N, N, N, N, N, N, 64, 320, N)),
    ("tokpool backward L = 0", "vc_mft_tokpool_bwd", (2, 121, 0, N, 64, N, N, N, N, N, 64, 320, N, 64, N, N, N, 0, N)),
    ("attention T = 1", "vc_mft_xattn_fwd", (2, 1, N, N, N, N, 0.35, N, N, N)),
    ("attention T = 17", "vc_mft_xattn_fwd", (2, 17, N, N, N, N, 0.35, N, N, N)),
    ("attention backward T = 1", "vc_mft_xattn_bwd", (2, 1, N, N, N, N, N, N, 0.35, N, N, N, N, N, 0, N)),
    ("attention backward T = 17", "vc_mft_xattn_bwd", (2, 17, N, N, N, N, N, N, 0.35, N, N, N, N, N, 0, N)),
    ("broadcast residual T = 0", "vc_mft_bcast_add_fwd", (2, 0, 64, N, N, N, N)),
    ("broadcast residual backward B = 0", "vc_mft_bcast_add_bwd", (0, 5, 64, N, N, N)),
    ("adam params not 16-B aligned", "vc_adam", (8, 4, N, N, N, N, N, N)),
    ("adam grads not 16-B aligned", "vc_adam", (8, N, 4, N, N, N, N, N)),
    ("adam moments not 16-B aligned", "vc_adam", (8, N, N, 8, N, N, N, N)),
    ("adam n < 0", "vc_adam", (-1, N, N, N, N, N, N, N)),
]


@pytest.mark.parametrize("what,name,args", REJECTED, ids=[r[0] for r in REJECTED])
def test_mft_host_side_rejections(what, name, args):
    assert _raw()[name](*args) == 1, what


def test_conv3d_ws_floats_sizes_the_partials_and_rejects_bad_shapes():
    raw = _raw()
    assert raw["vc_mft_conv3d_ws_floats"](2, 8, 11) == -1      # NC - 8 < 1
    assert raw["vc_mft_conv3d_ws_floats"](2, 30, 4) == -1      # P below the minimum
    assert raw["vc_mft_conv3d_ws_floats"](0, 30, 11) == -1
    assert raw["vc_mft_conv3d_ws_floats"](2, 9, 5) == 2 * 656          # one depth, one chunk per sample
    assert raw["vc_mft_conv3d_ws_floats"](64, 144, 11) == 64 * 17 * 656   # 136 depths in chunks of 8
    assert raw["vc_mft_conv3d_ws_floats"](1, 30, 28) > 0       # the largest patch the LDS plan takes
