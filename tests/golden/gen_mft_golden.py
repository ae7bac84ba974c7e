"""Generate the MFT golden vectors from the REFERENCE module (run in the build container only).

Imports `/root/reference/model/compare_method/MFT.py` (needs only torch + einops; its single `.cuda()` is in the
unused helper `INF`) and runs one train-mode forward / backward of `MFT` as `model_utils.py:364-376` builds it
(FM 16, HSIOnly False), built under `torch.manual_seed(0)`, with every `nn.Dropout.p` set to 0 (the reference's
dropout is random, so parity is only defined at p = 0).  Inputs ~ U[0, 1) from a seeded generator, labels in
[1, ncls), class weight 0 for class 0.  Numbers only are stored:

  mft_b4.npz      B=4, NC=30, NCLidar=1, P=11, 16 classes (HetConv g = 16)
  mft_odd_b4.npz  B=4, NC=11, NCLidar=2, P=7, 12 classes (g = 8, two LiDAR bands, widths no multiple of 4)
    "p:<key>" the initial state_dict, x1, x2, target, weight, logits, loss, "r:<key>" the BatchNorm running
    statistics after the forward, eval_logits (eval mode, same inputs, afterwards), seed (the input seed used)
  <name>_grads.npz  "g:<key>" every parameter gradient (a file of its own: the repository's 1 MiB limit per file)

The input seed advances until two conditions hold in float64 (the reference module cast to double):
  1. every pre-ReLU value of both ReLU stages has magnitude >= 1e-5, so an fp32 kernel's summation order cannot
     flip a decision;
  2. the reference's own fp32 gradients stay within a quarter of the test's rule
     (|g32 - g64| <= 1e-3 |g64| + 1e-5 gmax) against the float64 run.

Run:  python tests/golden/gen_mft_golden.py
"""
from __future__ import annotations

import copy
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/model/compare_method/MFT.py"


def _run(net, x1, x2, target, weight):
    pre = {}
    hooks = [net.conv5[1].register_forward_hook(lambda m, i, o: pre.__setitem__("conv5", o.detach())),
             net.conv6[1].register_forward_hook(lambda m, i, o: pre.__setitem__("conv6", o.detach()))]
    net.zero_grad()
    logits = net(x1, x2)
    loss = F.cross_entropy(logits, target, weight=weight)
    loss.backward()
    for h in hooks:
        h.remove()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p))
             for k, p in net.named_parameters()}
    return logits.detach(), loss.detach(), grads, pre


def make(name, B, NC, NCL, P, ncls, seed0=1):
    spec = importlib.util.spec_from_file_location("ref_mft", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(0)
    net0 = mod.MFT(patch_size=P, FM=16, NC=NC, NCLidar=NCL, Classes=ncls, HSIOnly=False)
    for m in net0.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    net0.train()
    sd0 = {k: v.detach().clone() for k, v in net0.state_dict().items()}
    weight = torch.ones(ncls)
    weight[0] = 0.0
    seed = seed0
    while True:
        g = torch.Generator().manual_seed(seed)
        x1 = torch.rand(B, NC, P, P, generator=g)
        x2 = torch.rand(B, NCL, P, P, generator=g)
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
    out = {"x1": x1.numpy(), "x2": x2.numpy(), "target": target.numpy(), "weight": weight.numpy(),
           "logits": logits.numpy(), "loss": np.float32(loss.item()), "seed": np.int64(seed)}
    for k, v in sd0.items():
        out["p:" + k] = v.numpy()
    for k, v in net.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"):
            out["r:" + k] = v.detach().numpy()
    net.eval()
    with torch.no_grad():
        out["eval_logits"] = net(x1, x2).numpy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    np.savez_compressed(os.path.join(HERE, name + "_grads.npz"), **{"g:" + k: v.numpy() for k, v in grads.items()})
    for f in (name + ".npz", name + "_grads.npz"):
        print("wrote", f, os.path.getsize(os.path.join(HERE, f)), "bytes; seed", seed, "loss", float(loss))


if __name__ == "__main__":
    make("mft_b4", 4, 30, 1, 11, 16)
    make("mft_odd_b4", 4, 11, 2, 7, 12)
