"""Measurement switches for the tools: VITCNN_<NAME> environment variables -> the program's module constants.

The product package reads no environment (vitcnn_amd/model.py, fusatnet.py: module constants, the lane schedule
family and FusAtNet's im2col route; the C ABI's kernel knobs exist only in libvitcnn_probe.so).  A tool that A/Bs
a switch (tools/ab_env.sh -> prof_step.py) imports this module first: it selects the probe library, copies every
VITCNN_* switch that is set onto the corresponding constant, and refuses a retired one.
"""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
_REPO = os.path.dirname(_HERE)
for _p in (_REPO, os.path.join(_REPO, "vit-cnn_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
PROBE_PATH = os.path.join(_REPO, "vit-cnn_amd", "vitcnn_amd", "libvitcnn_probe.so")
# the C ABI's kernel knobs (read by libvitcnn_probe.so only, common.h vc_knob)
PROBE_KNOBS = ("VITCNN_NL_LEGACY", "VITCNN_C2I_LDS", "VITCNN_TAP_NOSPLIT", "VITCNN_BN_PCAP", "VITCNN_BN_APPLY_ROWS", "VITCNN_BN_IM2COL",
               "VITCNN_BN_GLF", "VITCNN_SCAN_RBS", "VITCNN_SCAN_SELECT_RS", "VITCNN_SCAN_TAIL",
               "VITCNN_SPLITK_COMBINE", "VITCNN_LEGACY_COMBINE", "VITCNN_GEMM_PIPE", "VITCNN_GEMM_PIPE_SMALL",
               "VITCNN_PIPE_NS", "VITCNN_PIPE_BF_W8", "VITCNN_PIPE_F32_W8", "VITCNN_PIPE_SPLIT_BLOCKS", "VITCNN_PIPE_SPLIT_BELOW", "VITCNN_PIPE_SPLIT_FILL", "VITCNN_PIPE_KM", "VITCNN_GEMM_GROUP_MAXB",
               "VITCNN_TAP_TARGET", "VITCNN_TAP_PIPE", "VITCNN_CONV_PIPE_TILES_F", "VITCNN_CONV_PIPE_TILES_W",
               "VITCNN_CONV_PIPE_TILES_D", "VITCNN_CONV_PIPE_W8", "VITCNN_ATTN_BWD_WPB", "VITCNN_ATTN_FWD_WPB")


def use_probe():
    """bind lib() to libvitcnn_probe.so (call before the library is first used).  The product loader reads
    no environment; this tool-side switch honours VITCNN_LIB (an A/B build, tools/ab_steps.sh) or the probe."""
    from vitcnn_amd import _lib
    _lib.use_library_for_tools(os.environ.get("VITCNN_LIB", PROBE_PATH))


if "VITCNN_LIB" in os.environ or any(k in os.environ for k in PROBE_KNOBS):
    use_probe()

# env name -> (module, attribute, parser)
_FLAG = lambda v: v not in ("0", "", "false", "False")  # noqa: E731
SWITCHES = {
    "VITCNN_LANES": ("model", "_LANES", _FLAG),
    "VITCNN_LANES_BWD": ("model", "_LANES_BWD", _FLAG),
    "VITCNN_LANE_MAP": ("model", "_LANE_MAP", lambda v: [int(x) for x in v.split(",") if x]),
    "VITCNN_CH_LANE": ("model", "_CH_LANE", int),
    "VITCNN_CH_ORDERED": ("model", "_CH_ORDERED", _FLAG),
    "VITCNN_FUSAT_IM2COL": ("fusatnet", "_TAP_CONV", lambda v: not _FLAG(v)),
}
# switches of program forms that no longer exist ("Retired program forms"): an old A/B command line that
# sets one would compare two identical legs, so apply() refuses it
RETIRED = ("VITCNN_IMPLICIT_CONV", "VITCNN_TAP_DGRAD", "VITCNN_DEFER_WGRAD", "VITCNN_DEFER_WGRAD1",
           "VITCNN_GLOBAL_FIRST", "VITCNN_PG_LANE2", "VITCNN_BN_TICKETS", "VITCNN_BN_RELU_AFFINE",
           "VITCNN_ONE_PARAM_REDUCE", "VITCNN_BF16_MIN_K", "VITCNN_GEMM_GROUP", "VITCNN_GEMM_BNSTATS",
           "VITCNN_SCAN_FUSED", "VITCNN_GLF_FUSED", "VITCNN_ROW_CHAIN", "VITCNN_FUSAT_PAD_LIDAR")


def apply():
    import importlib
    gone = [k for k in RETIRED if k in os.environ]
    if gone:
        raise RuntimeError(f"{', '.join(gone)}: retired switch, the program has one form now (DESIGN.md, 'Retired "
                           f"program forms', names the last commit with both)")
    done = {}
    for env, (mod, attr, parse) in SWITCHES.items():
        v = os.environ.get(env)
        if v is None:
            continue
        m = importlib.import_module("vitcnn_amd." + mod)
        setattr(m, attr, parse(v))
        done[env] = getattr(m, attr)
    return done


APPLIED = apply()
