"""The HCTnet fixtures (tests/golden/hctnet_*.npz, made by tests/golden/gen_hctnet_golden.py from the reference module)
as tensors, shared by tests/test_hctnet_cpu.py and tests/test_hctnet.py; loaded once and left unchanged."""
import functools
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
KW = {"hctnet_a": dict(num_classes=16, num_tokens=6, heads=8),      # get_model's model (B 4, P 11)
      "hctnet_b": dict(num_classes=12, num_tokens=4, heads=8)}      # B 4, P 7
UNUSED = "transformer."     # the 12 parameters forward never touches
ZERO_GRAD_BIASES = ("conv3d_features.0.bias", "conv2d_features.0.bias", "conv2d_features2.0.bias")


@functools.lru_cache(maxsize=None)
def golden(name):
    """(state_dict in the reference's key order, running statistics after the step, gradients, tensors)"""
    def load(suffix):
        return np.load(os.path.join(HERE, "golden", name + suffix + ".npz"))

    z = load("")
    ps, gs = {}, {}
    for f in (z, load("_ct0"), load("_ct1")):
        ps.update({k[2:]: torch.from_numpy(f[k]) for k in f.files if k.startswith("p:")})
    for f in (load("_grads"), load("_grads_ct0"), load("_grads_ct1")):
        gs.update({k[2:]: torch.from_numpy(f[k]) for k in f.files})
    keys = [str(k) for k in z["keys"]]
    sd = {k: ps[k] for k in keys}
    gr = {k: gs[k] for k in keys if k in gs}
    run = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("r:")}
    t = {k: torch.from_numpy(z[k]) for k in ("x1", "x2", "target", "weight", "logits", "eval_logits")}
    t["loss"] = float(z["loss"])
    return sd, run, gr, t


def rel(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))
