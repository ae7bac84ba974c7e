"""Criteria on the MI355X: weighted cross-entropy (nn.CrossEntropyLoss(weight) of model_utils.py:311) and
Cross_fusion_CNN's three-output loss (losses.py:7-19)."""
from __future__ import annotations

import torch
import torch.nn as nn

from ._lib import lib


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index):
        B, ncls = logits.shape
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        s = torch.cuda.current_stream(logits.device).cuda_stream
        lib().vc_ce_fwd(B, ncls, logits.data_ptr(), target.data_ptr(), weight.data_ptr() if weight is not None else None,
                        ignore_index, loss.data_ptr(), s)
        ctx.save_for_backward(logits, target, weight if weight is not None else torch.empty(0))
        ctx.has_w = weight is not None
        ctx.ignore_index = ignore_index
        return loss

    @staticmethod
    def backward(ctx, gout):
        logits, target, weight = ctx.saved_tensors
        B, ncls = logits.shape
        gout = gout.detach().to(torch.float32).contiguous()
        dlog = torch.empty_like(logits)
        s = torch.cuda.current_stream(logits.device).cuda_stream
        lib().vc_ce_bwd(B, ncls, logits.data_ptr(), target.data_ptr(), weight.data_ptr() if ctx.has_w else None,
                        ctx.ignore_index, gout.data_ptr(), dlog.data_ptr(), s)
        return dlog, None, None, None


def ce_forward_backward(logits, target, weight, ignore_index=-100):
    """(loss, dlogits) of the weighted mean CE with d(loss) = 1, as one kernel on the current
    stream (the loss half of `fused_train_step`; vc_ce_fwd_bwd = vc_ce_fwd + vc_ce_bwd bit for bit)."""
    B, ncls = logits.shape
    s = torch.cuda.current_stream(logits.device).cuda_stream
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    dlog = torch.empty_like(logits)
    w = weight.data_ptr() if weight is not None else None
    lib().vc_ce_fwd_bwd(B, ncls, logits.data_ptr(), target.data_ptr(), w, ignore_index, loss.data_ptr(),
                        dlog.data_ptr(), s)
    return loss, dlog


class CrossEntropyLoss(nn.Module):
    """Drop-in for nn.CrossEntropyLoss(weight=...) with reduction='mean' (the reference's criterion)."""

    def __init__(self, weight=None, ignore_index: int = -100, reduction: str = "mean"):
        super().__init__()
        if reduction != "mean":
            raise ValueError("only reduction='mean' (the reference's setting) is implemented")
        self.register_buffer("weight", None if weight is None else weight.detach().to(torch.float32).clone())
        self.ignore_index = int(ignore_index)

    def forward(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if logits.device.type != "cuda":
            raise RuntimeError("ViT-CNN MI355X path: loss inputs must be on a ROCm (cuda) device")
        if logits.dim() != 2 or target.dim() != 1 or target.shape[0] != logits.shape[0]:
            raise RuntimeError(f"expected logits [B, C] and target [B], got {list(logits.shape)} / {list(target.shape)}")
        w = self.weight
        if w is not None:
            if w.numel() != logits.shape[1]:
                raise RuntimeError("weight tensor should be defined either for all classes or no classes")
            if w.device != logits.device:
                w = w.to(logits.device)
        return _CrossEntropyFn.apply(logits.to(torch.float32).contiguous(), target.to(torch.int64).contiguous(), w,
                                     self.ignore_index)


class _CrossFusionLossFn(torch.autograd.Function):
    """loss and the three logit gradients in one launch (vc_xfusion_loss_fwd_bwd); the gradients wait side by side
    in one buffer for the backward, which scales them by the incoming d(loss)"""

    @staticmethod
    def forward(ctx, o1, o2, o3, target, weight):
        B, ncls = o1.shape
        loss = torch.empty((), dtype=torch.float32, device=o1.device)
        grads = torch.empty(3, B, ncls, dtype=torch.float32, device=o1.device)
        s = torch.cuda.current_stream(o1.device).cuda_stream
        step = B * ncls * 4
        lib().vc_xfusion_loss_fwd_bwd(B, ncls, o1.data_ptr(), o2.data_ptr(), o3.data_ptr(), target.data_ptr(),
                                      weight.data_ptr() if weight is not None else None, loss.data_ptr(),
                                      grads.data_ptr(), grads.data_ptr() + step, grads.data_ptr() + 2 * step, s)
        ctx.save_for_backward(grads)
        return loss

    @staticmethod
    def backward(ctx, gout):
        (grads,) = ctx.saved_tensors
        g = grads * gout.detach().to(torch.float32)
        return g[0], g[1], g[2], None, None


class Cross_fusion_CNN_Loss(nn.Module):
    """Drop-in for the reference's Cross_fusion_CNN_Loss(weight) (losses.py:7-19): for output = (o1, o2, o3),
    weighted mean CE(o1, target) + mean((o1 - o2)^2) + mean((o1 - o3)^2), the means over all B * n_classes elements."""

    def __init__(self, weight=None):
        super().__init__()
        self.register_buffer("weight", None if weight is None else weight.detach().to(torch.float32).clone())

    def forward(self, output, target: torch.Tensor) -> torch.Tensor:
        o1, o2, o3 = output
        if o1.device.type != "cuda":
            raise RuntimeError("MDL-RS MI355X path: loss inputs must be on a ROCm (cuda) device")
        if o1.dim() != 2 or o2.shape != o1.shape or o3.shape != o1.shape or target.dim() != 1 or \
                target.shape[0] != o1.shape[0]:
            raise RuntimeError(f"expected three logits [B, C] and target [B], got {list(o1.shape)}, {list(o2.shape)}, "
                               f"{list(o3.shape)} / {list(target.shape)}")
        w = self.weight
        if w is not None:
            if w.numel() != o1.shape[1]:
                raise RuntimeError("weight tensor should be defined either for all classes or no classes")
            if w.device != o1.device:
                w = w.to(o1.device)
        o1, o2, o3 = (o.to(torch.float32).contiguous() for o in (o1, o2, o3))
        return _CrossFusionLossFn.apply(o1, o2, o3, target.to(device=o1.device, dtype=torch.int64).contiguous(), w)
