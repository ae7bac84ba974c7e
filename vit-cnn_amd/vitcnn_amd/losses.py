"""Criteria on the MI355X: weighted cross-entropy (nn.CrossEntropyLoss(weight) of model_utils.py:311),
Cross_fusion_CNN's three-output loss (losses.py:7-19) and EndNet's classification + reconstruction loss (losses.py:21-35)."""
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


class GLT_Loss(nn.Module):
    """The criterion of GLT-Net's training loop (the reference's utils.py:train_epoch adds the model's reconstruction
    loss to the cross entropy): for output = (x_cls, con_loss), CrossEntropyLoss(weight)(x_cls, target) + con_loss.
    On the device the cross entropy is `vc_ce_fwd` / `vc_ce_bwd` and the sum one scalar add, all on the current stream
    (graph-capturable); on CPU tensors it is the formula itself in torch (host-side checks only: the model has no CPU
    path)."""

    def __init__(self, weight=None):
        super().__init__()
        self.ce = CrossEntropyLoss(weight=weight)

    @property
    def weight(self):
        return self.ce.weight

    def forward(self, output, target: torch.Tensor) -> torch.Tensor:
        x_cls, con_loss = output
        if con_loss.dim() != 0:
            raise RuntimeError(f"expected (x_cls [B, C], con_loss []), got con_loss {list(con_loss.shape)}")
        if x_cls.device.type != "cuda":
            if x_cls.dim() != 2 or target.dim() != 1 or target.shape[0] != x_cls.shape[0]:
                raise RuntimeError(f"expected logits [B, C] and target [B], got {list(x_cls.shape)} / {list(target.shape)}")
            w = self.ce.weight
            return nn.functional.cross_entropy(x_cls, target.to(torch.int64), weight=None if w is None else w.to(x_cls)) + \
                con_loss
        return self.ce(x_cls, target.to(x_cls.device)) + con_loss.to(torch.float32)


class _EndNetLossFn(torch.autograd.Function):
    """loss and the three gradients in one launch (vc_endnet_loss_fwd_bwd); the gradients wait side by side in one
    buffer for the backward, which scales them by the incoming d(loss)"""

    @staticmethod
    def forward(ctx, out, de1, de2, x1, x2, target, weight):
        B, ncls = out.shape
        C1, C2 = de1.shape[1], de2.shape[1]
        loss = torch.empty((), dtype=torch.float32, device=out.device)
        grads = torch.empty(B * (ncls + C1 + C2), dtype=torch.float32, device=out.device)
        s = torch.cuda.current_stream(out.device).cuda_stream
        g0 = grads.data_ptr()
        lib().vc_endnet_loss_fwd_bwd(B, ncls, C1, C2, out.data_ptr(), target.data_ptr(),
                                     weight.data_ptr() if weight is not None else None, de1.data_ptr(), x1.data_ptr(),
                                     de2.data_ptr(), x2.data_ptr(), loss.data_ptr(), g0, g0 + 4 * B * ncls,
                                     g0 + 4 * B * (ncls + C1), s)
        ctx.save_for_backward(grads)
        ctx.dims = (B, ncls, C1, C2)
        return loss

    @staticmethod
    def backward(ctx, gout):
        (grads,) = ctx.saved_tensors
        B, ncls, C1, C2 = ctx.dims
        g = grads * gout.detach().to(torch.float32)
        a, b = B * ncls, B * (ncls + C1)
        return g[:a].view(B, ncls), g[a:b].view(B, C1), g[b:].view(B, C2), None, None, None, None


class EndNet_Loss(nn.Module):
    """Drop-in for the reference's EndNet_Loss(weight) (losses.py:21-35): for output = (out, de_x1, de_x2, ori_x1,
    ori_x2), weighted mean CE(out, target) + mean((de_x1 - ori_x1)^2) + mean((de_x2 - ori_x2)^2)."""

    def __init__(self, weight=None):
        super().__init__()
        self.register_buffer("weight", None if weight is None else weight.detach().to(torch.float32).clone())

    def forward(self, output, target: torch.Tensor) -> torch.Tensor:
        out, de1, de2, x1, x2 = output
        if out.device.type != "cuda":
            raise RuntimeError("EndNet MI355X path: loss inputs must be on a ROCm (cuda) device")
        B = out.shape[0]
        x1, x2 = x1.reshape(B, -1), x2.reshape(B, -1)
        if out.dim() != 2 or de1.shape != x1.shape or de2.shape != x2.shape or de1.dim() != 2 or target.dim() != 1 or \
                target.shape[0] != B:
            raise RuntimeError(f"expected out [B, C], two reconstructions shaped as their inputs and target [B], got "
                               f"{list(out.shape)}, {list(de1.shape)} / {list(x1.shape)}, {list(de2.shape)} / "
                               f"{list(x2.shape)}, {list(target.shape)}")
        w = self.weight
        if w is not None:
            if w.numel() != out.shape[1]:
                raise RuntimeError("weight tensor should be defined either for all classes or no classes")
            if w.device != out.device:
                w = w.to(out.device)
        out, de1, de2 = (o.to(torch.float32).contiguous() for o in (out, de1, de2))
        x1, x2 = (x.detach().to(torch.float32).contiguous() for x in (x1, x2))
        return _EndNetLossFn.apply(out, de1, de2, x1, x2, target.to(device=out.device, dtype=torch.int64).contiguous(), w)
