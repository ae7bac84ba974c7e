"""Generate the MHST golden vectors from the REFERENCE module (run in the build container only).

Imports the reference's `model/compare_method/MHST/MHST.py` (torch + einops; its `from timm.models.layers import
DropPath` is satisfied by an empty stand-in: DropPath is never instantiated at drop_path_rate 0) and runs one train-mode
forward / backward of `MHST` built under `torch.manual_seed(0)` with every `nn.Dropout.p` set to 0:

  mhst_a  the registry's model (model_utils.py:314-335) at 30 + 1 bands, 16 classes, B = 4
  mhst_b  11 + 2 bands, 12 classes, B = 3, en_depth 1, hsp_vit_depth 2

The gates' training noise is recorded without editing the reference: `HSPT._gumbel_sigmoid` is wrapped; the wrapper
seeds torch, draws g1, g2 with the function's own two `exponential_` calls and keeps g1 - g2, seeds torch again and
calls the original, which therefore draws the same numbers.  The float64 twin (the module cast to double) is fed the
recorded noise through a stand-in of that function.

The input / noise seed advances until, in float64:
  1. every pre-ReLU value of every BatchNorm has magnitude >= 1e-5;
  2. in every max-pool window with a positive maximum the runner-up is >= 1e-5 below it;
  3. every gate's pre-threshold value is >= 1e-3 in magnitude (training: (logits + noise) is checked; eval: logits);
  4. the fp32 reference and its float64 twin make the same gate decisions, and the reference's own fp32 gradients stay
     within a quarter of the test's rule (|g32 - g64| <= 1e-3 |g64| + 1e-5 gmax).

Stored (numbers only; files split below the repository's 1 MiB limit):
  <name>.npz        keys (the 338 / ... state_dict names in order), x1, x2, target, weight, noise [depth, B, 16],
                    out and loss (float64 twin, training), eval_out (float64 twin, eval, afterwards), ref_frac (the
                    reference's own fp32 gradients as a fraction of the rule), "r:<key>" BatchNorm running statistics
                    after the forward, seed
  <name>_p<i>.npz   "p:<key>" the initial state_dict (fp32, exact)
  <name>_g<i>.npz   "g:<key>" every parameter gradient (float64 twin, stored fp32)

Run:  python tests/golden/gen_mhst_golden.py   (VITCNN_REFERENCE names the reference tree)
"""
from __future__ import annotations

import copy
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("VITCNN_REFERENCE", "/root/reference")
LIMIT = 1 << 20
CHUNK = 900 * 1024


def _load():
    if "timm" not in sys.modules:
        timm, models, layers = (types.ModuleType(n) for n in ("timm", "timm.models", "timm.models.layers"))
        layers.DropPath = None
        timm.models, models.layers = models, layers
        sys.modules.update({"timm": timm, "timm.models": models, "timm.models.layers": layers})
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from model.compare_method.MHST import HSPT, MHST
    return MHST, HSPT


class Noise:
    """the wrapper around HSPT._gumbel_sigmoid: records (fp32 run) or replays (float64 twin) the gates' noise"""

    def __init__(self, hspt, seed):
        self.hspt, self.orig, self.seed = hspt, hspt._gumbel_sigmoid, seed
        self.rec, self.values = [], []
        self.mode = "record"

    def __call__(self, logits, tau=1, hard=True, eps=1e-10, training=True, threshold=0.5):
        i = len(self.values)
        if not training:
            self.values.append(logits.detach().double())
            return self.orig(logits, tau, hard, eps, training, threshold)
        if self.mode == "record":
            s = self.seed * 1000 + i
            torch.manual_seed(s)
            g1 = -torch.empty_like(logits).exponential_().log()
            g2 = -torch.empty_like(logits).exponential_().log()
            self.rec.append((g1 - g2).detach().clone())
            self.values.append((logits + self.rec[-1]).detach().double())
            torch.manual_seed(s)
            return self.orig(logits, tau, hard, eps, training, threshold)
        v = logits + self.rec[i].to(logits.dtype)
        self.values.append(v.detach().double())
        y = torch.sigmoid(v / tau)
        return (v > 0).to(logits.dtype) - y.detach() + y

    def begin(self, mode):
        self.mode, self.values = mode, []
        if mode == "record":
            self.rec = []


def _run(net, noise, mode, x1, x2, target, weight):
    bn, pools = {}, {}
    hooks = []
    for k, m in net.named_modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            hooks.append(m.register_forward_hook(lambda m, i, o, k=k: bn.__setitem__(k, o.detach())))
        if isinstance(m, torch.nn.MaxPool2d):
            hooks.append(m.register_forward_hook(lambda m, i, o, k=k: pools.__setitem__(k, i[0].detach())))
    noise.begin(mode)
    net.zero_grad()
    out = net(x1, x2)
    loss = F.cross_entropy(out, target, weight=weight)
    loss.backward()
    for h in hooks:
        h.remove()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p))
             for k, p in net.named_parameters()}
    return out.detach(), loss.detach(), grads, bn, pools, list(noise.values)


def pool_gap(x):
    """the smallest (max - runner-up) over the 2x2 windows whose max is positive"""
    B, C, H, W = x.shape
    w = x.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4)
    top = w.topk(2, dim=1).values
    pos = top[:, 0] > 0
    return float((top[pos, 0] - top[pos, 1]).min()) if bool(pos.any()) else float("inf")


def _save(fname, arrays):
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < LIMIT, (fname, size)
    print("wrote", fname, size, "bytes")
    return size


def _save_chunks(stem, tag, tensors):
    part, size, idx, total = {}, 0, 0, 0
    for k, v in tensors.items():
        a = v.detach().to(torch.float32).numpy() if v.dtype.is_floating_point else v.numpy()
        if part and size + a.nbytes > CHUNK:
            total += _save(f"{stem}_{tag}{idx}.npz", part)
            part, size, idx = {}, 0, idx + 1
        assert a.nbytes <= CHUNK, (k, a.nbytes)
        part[f"{tag}:{k}"] = a
        size += a.nbytes
    total += _save(f"{stem}_{tag}{idx}.npz", part)
    return total


def make(name, l1, l2, ncls, B, en_depth, hs_depth, n_keys, seed0=1):
    MHST, HSPT = _load()
    torch.manual_seed(0)
    net0 = MHST.MHST(l1=l1, l2=l2, patch_size=8, num_patches=64, num_classes=ncls, encoder_embed_dim=64,
                     en_depth=en_depth, en_heads=4, mlp_dim=8, dropout=0.1, emb_dropout=0.1, coefficient_hsi=0.6,
                     coefficient_vit=0.7, hsp_vit_depth=hs_depth, hsp_vit_num_heads=16, head_tau=5, use_head_select=True,
                     vit_qkv_bias=False, mlp_ratio=4, attnproj_mlp_drop=0.1, attn_drop=0.1)
    for m in net0.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    net0.train()
    sd0 = {k: v.detach().clone() for k, v in net0.state_dict().items()}
    assert n_keys is None or len(sd0) == n_keys, len(sd0)
    print(name, "parameters", sum(p.numel() for p in net0.parameters()), "keys", len(sd0))
    weight = torch.ones(ncls)
    weight[0] = 0.0
    seed = seed0
    while True:
        g = torch.Generator().manual_seed(seed)
        x1 = torch.rand(B, l1, 8, 8, generator=g)
        x2 = torch.rand(B, l2, 8, 8, generator=g)
        target = torch.randint(1, ncls, (B,), generator=g)
        noise = Noise(HSPT, seed)
        HSPT._gumbel_sigmoid = noise
        try:
            net, net64 = copy.deepcopy(net0), copy.deepcopy(net0).double()
            _, _, grads, _, _, gate32 = _run(net, noise, "record", x1, x2, target, weight)
            out64, loss64, g64, bn64, pools64, gate64 = _run(net64, noise, "replay", x1.double(), x2.double(), target,
                                                             weight.double())
            net64.eval()
            noise.begin("replay")
            with torch.no_grad():
                eval64 = net64(x1.double(), x2.double())
            gate_eval = list(noise.values)
        finally:
            HSPT._gumbel_sigmoid = noise.orig
        min_pre = min(float(v.abs().min()) for v in bn64.values())
        gap = min(pool_gap(v) for v in pools64.values())
        min_gate = min(float(v.abs().min()) for v in gate64)
        min_gate_eval = min(float(v.abs().min()) for v in gate_eval)
        same = all(bool(((a > 0) == (b > 0)).all()) for a, b in zip(gate32, gate64))
        gmax = max(float(v.norm()) for v in g64.values())
        frac = max(float((grads[k].double() - g64[k]).norm()) / (1e-3 * float(g64[k].norm()) + 1e-5 * gmax)
                   for k in g64)
        print(f"{name}: seed {seed}: pre-ReLU {min_pre:.3e}, pool gap {gap:.3e}, gate {min_gate:.3e} / eval "
              f"{min_gate_eval:.3e}, decisions equal {same}, fp32 gradients at {frac:.4f} of the rule")
        if min_pre >= 1e-5 and gap >= 1e-5 and min_gate >= 1e-3 and min_gate_eval >= 1e-3 and same and frac <= 0.25:
            break
        seed += 1
    out = {"keys": np.array(list(sd0.keys())), "x1": x1.numpy(), "x2": x2.numpy(), "target": target.numpy(),
           "weight": weight.numpy(), "noise": torch.stack(noise.rec).numpy(), "out": out64.numpy(),
           "loss": np.float64(loss64.item()), "eval_out": eval64.numpy(), "ref_frac": np.float64(frac),
           "seed": np.int64(seed)}
    for k, v in net64.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            out["r:" + k] = v.detach().to(torch.float32).numpy()
    total = _save(name + ".npz", out)
    total += _save_chunks(name, "p", sd0)
    total += _save_chunks(name, "g", g64)
    print(name, "seed", seed, "loss", float(loss64), "bytes", total)


if __name__ == "__main__":
    make("mhst_a", 30, 1, 16, 4, 5, 8, 338)
    make("mhst_b", 11, 2, 12, 3, 1, 2, None)
