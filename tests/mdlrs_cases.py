"""The MDL-RS fixtures of tests/golden (gen_mdlrs_golden.py), shared by test_mdlrs_cpu.py and test_mdlrs.py."""
import functools
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
A = dict(B=4, C1=30, C2=1, P=7, ncls=16)
B_ = dict(B=3, C1=13, C2=2, P=5, ncls=12)
# fixture -> (class name, case)
CASES = {"mdlrs_early_a": ("Early_fusion_CNN", A), "mdlrs_middle_a": ("Middle_fusion_CNN", A),
         "mdlrs_late_a": ("Late_fusion_CNN", A), "mdlrs_cross_a": ("Cross_fusion_CNN", A),
         "mdlrs_early_b": ("Early_fusion_CNN", B_), "mdlrs_cross_b": ("Cross_fusion_CNN", B_)}
N_KEYS = {"Early_fusion_CNN": 44, "Middle_fusion_CNN": 72, "Late_fusion_CNN": 86, "Cross_fusion_CNN": 72}


@functools.lru_cache(maxsize=None)
def golden(name):
    """(state dict, running statistics after the forward, gradients, tensors); the tensors' "logits" and
    "eval_logits" are tuples (of three for Cross_fusion_CNN, of one otherwise)"""
    z = np.load(os.path.join(HERE, "golden", name + ".npz"))
    zg = np.load(os.path.join(HERE, "golden", name + "_grads.npz"))
    zp = np.load(os.path.join(HERE, "golden", str(z["params_from"]) + ".npz")) if "params_from" in z.files else z
    sd = {k[2:]: torch.from_numpy(zp[k]) for k in zp.files if k.startswith("p:")}
    run = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("r:")}
    gr = {k[2:]: torch.from_numpy(zg[k]) for k in zg.files}
    t = {k: torch.from_numpy(z[k]) for k in ("x1", "x2", "target", "weight")}
    for key in ("logits", "eval_logits"):
        t[key] = tuple(torch.from_numpy(z[key + s]) for s in ("", "2", "3") if key + s in z.files)
    t["loss"] = float(z["loss"])
    return sd, run, gr, t


def build(name, **extra):
    """the product module of a fixture's class and case (not loaded, on the CPU)"""
    from vitcnn_amd import mdlrs
    cls, case = CASES[name]
    return getattr(mdlrs, cls)(case["C1"], case["C2"], case["ncls"], **extra)
