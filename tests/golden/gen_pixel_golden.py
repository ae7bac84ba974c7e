"""Generate the EndNet / SpectralFormer golden vectors from the REFERENCE modules (run in the build container only).

Imports `/root/reference/model/compare_method/EndNet.py`, `.../spectralformer.py` (torch + einops) and
`/root/reference/losses.py` and runs one train-mode forward / backward of each net as `model_utils.py:119-128` /
`:377-399` build it (SpectralFormer with dropout 0, so the fixture is deterministic), built under
`torch.manual_seed(0)`.  Inputs ~ U[0, 1) from a seeded generator as pixel rows [B, C], labels in [1, ncls), class
weight 0 for class 0; the criterion is the reference's EndNet_Loss / the weighted cross entropy.  Numbers only:

  case A  B=4, 30+1 bands, 16 classes   endnet_a, spectralformer_a
  case B  B=3, 13+2 bands, 12 classes   endnet_b, spectralformer_b
    <name>.npz: "p:<key>" the initial state_dict, x1, x2, target, weight, logits (EndNet: also de_x1, de_x2), loss,
      "r:<key>" (EndNet) the BatchNorm running statistics and num_batches_tracked after the forward, eval_logits
      (eval mode, same inputs, afterwards; EndNet: also eval_de_x1, eval_de_x2), seed (the input seed used)
    <name>_grads.npz: "g:<key>" every parameter gradient (zeros for the parameters the forward never applies)

EndNet: the input seed advances from 1 until, in float64 (the reference module cast to double), every BatchNorm
output in front of a ReLU has magnitude >= 1e-5, so an fp32 kernel's summation order cannot flip a ReLU decision
(the MDL-RS generator's rule).  It fails loudly if no seed up to 50 passes.

Run:  python tests/golden/gen_pixel_golden.py
"""
from __future__ import annotations

import copy
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = "/root/reference/model/compare_method"
REF_LOSS = "/root/reference/losses.py"


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(net, crit, x1, x2, target, endnet):
    rec = {"pre": float("inf")}

    def bn_hook(m, i, o):
        rec["pre"] = min(rec["pre"], float(o.detach().abs().min()))

    hooks = [m.register_forward_hook(bn_hook) for m in net.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    net.zero_grad()
    out = net(x1, x2)
    loss = crit(out, target)
    loss.backward()
    for h in hooks:
        h.remove()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p))
             for k, p in net.named_parameters()}
    outs = tuple(o.detach() for o in out[:3]) if endnet else (out.detach(),)
    return outs, loss.detach(), grads, rec


def make(name, cls, B, C1, C2, ncls):
    endnet = cls == "EndNet"
    lossmod = _load(REF_LOSS, "ref_losses")
    torch.manual_seed(0)
    if endnet:
        net0 = _load(os.path.join(REF_DIR, "EndNet.py"), "ref_endnet").EndNet(C1, C2, ncls)
    else:
        net0 = _load(os.path.join(REF_DIR, "spectralformer.py"), "ref_spectralformer").SpectralFormer(
            image_size=1, near_band=1, num_patches=C1 + C2, num_classes=ncls, dim=64, depth=5, heads=4, mlp_dim=8,
            dropout=0.0, emb_dropout=0.0, mode="ViT")
    net0.train()
    sd0 = {k: v.detach().clone() for k, v in net0.state_dict().items()}
    weight = torch.ones(ncls)
    weight[0] = 0.0

    def criterion(w):
        return lossmod.EndNet_Loss(weight=w) if endnet else torch.nn.CrossEntropyLoss(weight=w)

    for seed in range(1, 51):
        g = torch.Generator().manual_seed(seed)
        x1 = torch.rand(B, C1, generator=g)
        x2 = torch.rand(B, C2, generator=g)
        target = torch.randint(1, ncls, (B,), generator=g)
        net = copy.deepcopy(net0)
        outs, loss, grads, _ = _run(net, criterion(weight), x1, x2, target, endnet)
        if not endnet:
            break
        _, _, _, rec = _run(copy.deepcopy(net0).double(), criterion(weight.double()), x1.double(), x2.double(), target,
                            endnet)
        print(f"{name}: seed {seed}: smallest |BN output| in float64 {rec['pre']:.3e}")
        if rec["pre"] >= 1e-5:
            break
    else:
        raise SystemExit(f"{name}: no input seed in 1..50 keeps every BatchNorm output 1e-5 away from 0")
    out = {"x1": x1.numpy(), "x2": x2.numpy(), "target": target.numpy(), "weight": weight.numpy(),
           "loss": np.float32(loss.item()), "seed": np.int64(seed)}
    for k, o in zip(("logits", "de_x1", "de_x2"), outs):
        out[k] = o.numpy()
    for k, v in sd0.items():
        out["p:" + k] = v.numpy()
    for k, v in net.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"):
            out["r:" + k] = v.detach().numpy()
    net.eval()
    with torch.no_grad():
        ev = net(x1, x2)
        for k, o in zip(("eval_logits", "eval_de_x1", "eval_de_x2"), ev[:3] if endnet else (ev,)):
            out[k] = o.numpy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    np.savez_compressed(os.path.join(HERE, name + "_grads.npz"), **{"g:" + k: v.numpy() for k, v in grads.items()})
    for f in (name + ".npz", name + "_grads.npz"):
        size = os.path.getsize(os.path.join(HERE, f))
        assert size < (1 << 20), (f, size)
        print("wrote", f, size, "bytes; seed", seed, "loss", float(loss))


if __name__ == "__main__":
    A = dict(B=4, C1=30, C2=1, ncls=16)
    Bc = dict(B=3, C1=13, C2=2, ncls=12)
    make("endnet_a", "EndNet", **A)
    make("endnet_b", "EndNet", **Bc)
    make("spectralformer_a", "SpectralFormer", **A)
    make("spectralformer_b", "SpectralFormer", **Bc)
