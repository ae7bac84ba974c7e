"""The recorded launch sequences (tests/golden/launch_trace.json, written by tests/golden/gen_launch_trace.py): one
training forward + backward of each comparison model whose program is built from `program.Program`'s shared helpers, at
the smallest shapes its tests use, B = 2, train mode, the models' dropout 0.1 where they have one, under
torch.manual_seed(0), on a freshly built model (the cached workspace's size is an argument of the launches)."""
import json
import os

import torch

from helpers import GOLDEN, launch_trace

FIXTURE = os.path.join(GOLDEN, "launch_trace.json")
B = 2


def _mhst():
    import mhst_cases
    return mhst_cases.build("mhst_b", p_zero=False), (11, 8, 8), (2, 8, 8)


def _glt():
    import glt_cases
    return glt_cases.build("glt_b", p_zero=False), (11, 12, 12), (2, 12, 12)


def _hct():
    from vitcnn_amd.hctnet import HCTnet
    return HCTnet(num_classes=12, num_tokens=4, heads=8), (3, 7, 7), (1, 7, 7)


def _mft():
    from vitcnn_amd.mft import MFT
    return MFT(patch_size=7, FM=16, NC=11, NCLidar=1, Classes=12, HSIOnly=False), (11, 7, 7), (1, 7, 7)


def _cross_fusion():
    from vitcnn_amd.mdlrs import P_MIN, Cross_fusion_CNN
    return Cross_fusion_CNN(5, 1, 3), (5, P_MIN, P_MIN), (1, P_MIN, P_MIN)


def _fusatnet():
    from vitcnn_amd.fusatnet import FusAtNet
    return FusAtNet(144, 1, 16), (144, 11, 11), (1, 11, 11)


CASES = {"mhst_b": _mhst, "glt_b": _glt, "hctnet": _hct, "mft": _mft, "cross_fusion": _cross_fusion,
         "fusatnet": _fusatnet}


def record(name, dev="cuda"):
    """the launch trace of one training forward + backward of case `name`, after the fixture's JSON round trip"""
    from vitcnn_amd._lib import lib
    torch.manual_seed(0)
    m, s1, s2 = CASES[name]()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):   # the MHST / GLT registry's value already
            mod.p = 0.1
    m = m.to(dev).train()
    g = torch.Generator().manual_seed(5)
    x1, x2 = torch.rand(B, *s1, generator=g).to(dev), torch.rand(B, *s2, generator=g).to(dev)
    torch.manual_seed(0)
    with launch_trace(lib()) as trace:
        outs = m(x1, x2)
        outs = [o for o in ([outs] if torch.is_tensor(outs) else outs) if torch.is_tensor(o) and o.requires_grad]
        sum(o.sum() for o in outs).backward()
        torch.cuda.synchronize()
    return json.loads(json.dumps(trace))


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)
