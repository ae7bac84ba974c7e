"""The recorded lane DAGs of the ViT-CNN step (tests/golden/vitcnn_lane_trace.json, written by tests/golden/
gen_vitcnn_lane_trace.py): per case one `fused_train_step` (training forward, CrossEntropyLoss, backward) at B = 2 on a
freshly built, hash-initialised model, as helpers.LaneRecorder notes it; "eval" is one eval-mode forward of the first
case under no_grad.  (c1, c2, P, ncls), precision, module constants of vitcnn_amd.model set for the run."""
import json
import os

import torch

from helpers import GOLDEN, lane_trace

FIXTURE = os.path.join(GOLDEN, "vitcnn_lane_trace.json")
B = 2
TAG = "lanes.b2"
CASES = {
    "c144_fp32": ((144, 1, 9, 16), "fp32", {}),                        # the default path
    "c144_bf16": ((144, 1, 9, 16), "bf16", {}),
    "c144_fp32_lanes_bwd_off": ((144, 1, 9, 16), "fp32", {"_LANES_BWD": False}),   # the non-deferring backward
    "c30_fp32": ((30, 1, 7, 16), "fp32", {}),    # row chains refused, unaligned 1x1 fusion (vc_bn_forward_ex)
    "c5_2_fp32": ((5, 2, 7, 4), "fp32", {}),     # the two-band LiDAR path
    "eval": ((144, 1, 9, 16), "fp32", {}),
}


def record(name, dev="cuda"):
    """the lane DAG of case `name`, after the fixture's JSON round trip"""
    import vitcnn_amd.model as VM
    from vitcnn_amd import CrossEntropyLoss, Multimodality_Mamba, fused_train_step
    from vitcnn_amd.hashinit import fill_module_, synthetic_batch
    (c1, c2, P, ncls), precision, consts = CASES[name]
    m = Multimodality_Mamba(P, 1, 1, c1, c2, 32, ncls, "multi_clock_gate", precision=precision)
    fill_module_(m)
    m = m.to(dev)
    hsi, lidar, target = (torch.from_numpy(a).to(dev) for a in synthetic_batch(TAG, B, c1, c2, P, ncls))
    saved = {k: getattr(VM, k) for k in consts}
    for k, v in consts.items():
        setattr(VM, k, v)
    try:
        with lane_trace() as rec:
            if name == "eval":
                with torch.no_grad():
                    m.eval()(hsi, lidar)
            else:
                fused_train_step(m.train(), CrossEntropyLoss(), hsi, lidar, target)
            torch.cuda.synchronize()
    finally:
        for k, v in saved.items():
            setattr(VM, k, v)
    return json.loads(json.dumps(rec.nodes))


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)
