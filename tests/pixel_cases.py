"""The EndNet / SpectralFormer fixtures of tests/golden (gen_pixel_golden.py), shared by test_pixel_cpu.py and
test_pixel.py."""
import functools
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
A = dict(B=4, C1=30, C2=1, ncls=16)
B_ = dict(B=3, C1=13, C2=2, ncls=12)
# fixture -> (class name, case)
CASES = {"endnet_a": ("EndNet", A), "endnet_b": ("EndNet", B_),
         "spectralformer_a": ("SpectralFormer", A), "spectralformer_b": ("SpectralFormer", B_)}
N_KEYS = {"EndNet": 93, "SpectralFormer": 69}
OUT_KEYS = {"EndNet": ("logits", "de_x1", "de_x2"), "SpectralFormer": ("logits",)}


@functools.lru_cache(maxsize=None)
def golden(name):
    """(state dict, running statistics after the forward, gradients, tensors); the tensors' "outs" and "eval_outs" are
    tuples (out, de_x1, de_x2) for EndNet and (logits,) for SpectralFormer"""
    cls, _ = CASES[name]
    z = np.load(os.path.join(HERE, "golden", name + ".npz"))
    zg = np.load(os.path.join(HERE, "golden", name + "_grads.npz"))
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p:")}
    run = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("r:")}
    gr = {k[2:]: torch.from_numpy(zg[k]) for k in zg.files}
    t = {k: torch.from_numpy(z[k]) for k in ("x1", "x2", "target", "weight")}
    t["outs"] = tuple(torch.from_numpy(z[k]) for k in OUT_KEYS[cls])
    t["eval_outs"] = tuple(torch.from_numpy(z["eval_" + k]) for k in OUT_KEYS[cls])
    t["loss"] = float(z["loss"])
    return sd, run, gr, t


def build(name, dropout=0.0):
    """the product module of a fixture's class and case (not loaded, on the CPU); the fixtures hold dropout 0"""
    import vitcnn_amd
    cls, case = CASES[name]
    if cls == "EndNet":
        return vitcnn_amd.EndNet(case["C1"], case["C2"], case["ncls"])
    return spectralformer(case["C1"] + case["C2"], case["ncls"], dropout)


def spectralformer(num_patches, ncls, dropout=0.0):
    """SpectralFormer as get_model builds it (model_utils.py:377-399), with the given dropout"""
    import vitcnn_amd
    return vitcnn_amd.SpectralFormer(image_size=1, near_band=1, num_patches=num_patches, num_classes=ncls, dim=64,
                                     depth=5, heads=4, mlp_dim=8, dropout=dropout, emb_dropout=dropout, mode="ViT")
