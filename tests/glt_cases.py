"""The GLT-Net fixtures (tests/golden/gen_glt_golden.py) and the model each was made with, shared by tests/test_glt*.py."""
import glob
import os

import numpy as np
import torch

from helpers import GOLDEN

REGISTRY = dict(encoder_embed_dim=64, decoder_embed_dim=32, en_heads=4, de_heads=4, mlp_dim=8, dim_head=16, dropout=0.1,
                emb_dropout=0.1)
CASES = {
    "glt_a": dict(l1=30, l2=1, patch_size=8, num_patches=64, num_classes=16, en_depth=5, de_depth=5),
    "glt_b": dict(l1=11, l2=2, patch_size=4, num_patches=16, num_classes=12, en_depth=1, de_depth=2),
}
_CACHE = {}


def load(name):
    """{"keys", "state" (initial state_dict, fp32), "grads" (the float64 twin's), "running" (BatchNorm running statistics
    and num_batches_tracked after the training forward), and the scalars / arrays of <name>.npz as tensors}; loaded once"""
    if name not in _CACHE:
        z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
        d = {k: torch.from_numpy(np.asarray(z[k])) for k in z.files if k != "keys" and not k.startswith("r:")}
        d["keys"] = [str(k) for k in z["keys"]]
        d["running"] = {k[2:]: torch.from_numpy(np.asarray(z[k])) for k in z.files if k.startswith("r:")}
        for tag, field in (("p", "state"), ("g", "grads")):
            d[field] = {}
            for path in sorted(glob.glob(os.path.join(GOLDEN, f"{name}_{tag}[0-9].npz"))):
                zz = np.load(path, allow_pickle=False)
                d[field].update({k[2:]: torch.from_numpy(np.asarray(zz[k])) for k in zz.files})
        assert list(d["state"]) == d["keys"]
        _CACHE[name] = d
    return _CACHE[name]


def build(name, p_zero=True):
    """the product model of a case, constructed under torch.manual_seed(0) as the fixture's was (CPU, train mode)"""
    from vitcnn_amd.glt import GLT
    torch.manual_seed(0)
    m = GLT(**CASES[name], **REGISTRY)
    if p_zero:
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
    return m.train()


def grad_rule_fraction(got, want):
    """the worst |g - g_ref| / (1e-3 |g_ref| + 1e-5 gmax) over all parameters (norms per tensor), and its key"""
    gmax = max(float(v.double().norm()) for v in want.values())
    worst, where = 0.0, None
    for k, w in want.items():
        w = w.double()
        f = float((got[k].double().cpu().reshape(w.shape) - w).norm()) / (1e-3 * float(w.norm()) + 1e-5 * gmax)
        if f > worst:
            worst, where = f, k
    return worst, where
