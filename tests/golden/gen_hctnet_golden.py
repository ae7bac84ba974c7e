"""Generate the HCTnet golden vectors from the REFERENCE module (run in the build container only).

Imports the reference's `model/compare_method/HCTnet.py` (torch + einops; `torchvision` and `torchsummary` are
imported there and never used, and neither is installed, so empty modules stand in for them) and runs one train-mode
forward / backward of `HCTnet` as `model_utils.py:351-363` builds it (`num_tokens`, `heads=8`), built under
`torch.manual_seed(0)`, with every `nn.Dropout.p` set to 0 (the reference's dropout is random, so parity is only
defined at p = 0).  Inputs ~ U[0, 1) from a seeded generator, labels in [1, ncls), class weight 0 for class 0.
Numbers only are stored:

  hctnet_a  B=4, P=11, 16 classes, 6 tokens (get_model's model)
  hctnet_b  B=4, P=7, 12 classes, 4 tokens
    <name>.npz            "keys" (the state_dict's 77 names in order), "p:<key>" the initial state_dict without the
                          cross-token matrices, x1, x2, target, weight, logits, loss, "r:<key>" the BatchNorm running
                          statistics after the forward, eval_logits (eval mode, same inputs, afterwards), seed
    <name>_ct<d>.npz      "p:<key>" direction d's to_q / to_kv / to_out matrices
    <name>_grads.npz      "g:<key>" every parameter gradient but the cross-token matrices'
    <name>_grads_ct<d>.npz  "g:<key>" those
  (the parameters are 1.31 MB and so are the gradients; the repository's limit is 1 MiB per file)

The input seed advances until two conditions hold in float64 (the reference module cast to double):
  1. every pre-ReLU value of the three BatchNorms has magnitude >= 1e-5, so an fp32 kernel's summation order cannot
     flip a decision;
  2. the reference's own fp32 gradients stay within a quarter of the test's rule
     (|g32 - g64| <= 1e-3 |g64| + 1e-5 gmax) against the float64 run.

Run:  python tests/golden/gen_hctnet_golden.py   (VITCNN_REFERENCE names the reference tree)
"""
from __future__ import annotations

import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(os.environ.get("VITCNN_REFERENCE", "/root/reference"), "model", "compare_method", "HCTnet.py")
LIMIT = 1 << 20


def _load():
    for name in ("torchvision", "torchsummary"):   # imported by the reference file, never used
        if name not in sys.modules:
            stub = types.ModuleType(name)
            stub.summary = None
            sys.modules[name] = stub
    spec = importlib.util.spec_from_file_location("ref_hctnet", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(net, x1, x2, target, weight):
    pre = {}
    stages = {"conv3d": net.conv3d_features[1], "conv2d": net.conv2d_features[1], "conv2d2": net.conv2d_features2[1]}
    hooks = [m.register_forward_hook(lambda m, i, o, k=k: pre.__setitem__(k, o.detach())) for k, m in stages.items()]
    net.zero_grad()
    logits = net(x1, x2)
    loss = F.cross_entropy(logits, target, weight=weight)
    loss.backward()
    for h in hooks:
        h.remove()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p))
             for k, p in net.named_parameters()}
    return logits.detach(), loss.detach(), grads, pre


def ct_file(key):
    """the index d of the cross-token direction whose big matrix `key` is, or None"""
    for d in (0, 1):
        pfx = f"fusion_encoder.layers.0.2.layers.0.{d}.fn.fn."
        if key.startswith(pfx) and key.endswith(".weight") and "norm" not in key:
            return d
    return None


def _save(fname, arrays):
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < LIMIT, (fname, size)
    print("wrote", fname, size, "bytes")


def make(name, B, P, ncls, L, seed0=1):
    mod = _load()
    torch.manual_seed(0)
    net0 = mod.HCTnet(num_classes=ncls, num_tokens=L, heads=8)
    for m in net0.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    net0.train()
    sd0 = {k: v.detach().clone() for k, v in net0.state_dict().items()}
    assert len(sd0) == 77
    weight = torch.ones(ncls)
    weight[0] = 0.0
    seed = seed0
    while True:
        g = torch.Generator().manual_seed(seed)
        x1 = torch.rand(B, 3, P, P, generator=g)
        x2 = torch.rand(B, 1, P, P, generator=g)
        target = torch.randint(1, ncls, (B,), generator=g)
        net = copy.deepcopy(net0)
        net64 = copy.deepcopy(net0).double()
        logits, loss, grads, _ = _run(net, x1, x2, target, weight)
        _, _, g64, pre64 = _run(net64, x1.double(), x2.double(), target, weight.double())
        min_pre = min(float(v.abs().min()) for v in pre64.values())
        gmax = max(float(v.norm()) for v in g64.values())
        frac = max(float((grads[k].double() - g64[k]).norm()) / (1e-3 * float(g64[k].norm()) + 1e-5 * gmax)
                   for k in g64)
        print(f"{name}: seed {seed}: smallest pre-ReLU {min_pre:.3e}, fp32 gradients at {frac:.4f} of the rule")
        if min_pre >= 1e-5 and frac <= 0.25:
            break
        seed += 1
    out = {"keys": np.array(list(sd0.keys())), "x1": x1.numpy(), "x2": x2.numpy(), "target": target.numpy(),
           "weight": weight.numpy(), "logits": logits.numpy(), "loss": np.float32(loss.item()), "seed": np.int64(seed)}
    ct = ({}, {})
    gout, gct = {}, ({}, {})
    for k, v in sd0.items():
        d = ct_file(k)
        (out if d is None else ct[d])["p:" + k] = v.numpy()
    for k, v in net.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"):
            out["r:" + k] = v.detach().numpy()
    for k, v in grads.items():
        d = ct_file(k)
        (gout if d is None else gct[d])["g:" + k] = v.numpy()
    net.eval()
    with torch.no_grad():
        out["eval_logits"] = net(x1, x2).numpy()
    _save(name + ".npz", out)
    _save(name + "_grads.npz", gout)
    for d in (0, 1):
        assert len(ct[d]) == 3 and len(gct[d]) == 3
        _save(f"{name}_ct{d}.npz", ct[d])
        _save(f"{name}_grads_ct{d}.npz", gct[d])
    print(name, "seed", seed, "loss", float(loss))


if __name__ == "__main__":
    make("hctnet_a", 4, 11, 16, 6)
    make("hctnet_b", 4, 7, 12, 4)
