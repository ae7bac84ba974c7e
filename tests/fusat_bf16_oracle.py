"""ORACLE -- test infrastructure only.  FusAtNet with bf16 operands on its 3x3 convolutions, on the CPU.

`forward(sd, x1, x2, train, rounding=True)` runs `oracle.fusat_oracle.forward` with that module's `F.conv2d`
substituted for the duration of the call: every 3x3 convolution becomes `RoundedConv3x3`, the arithmetic of
`precision="bf16"` --

  forward   y  = conv(r(x), r(w)) + b
  wgrad     dw = corr(r(x), r(dy))
  dgrad     dx = conv^T(r(dy), r(w))
  bias      db = sum(dy)                      (unrounded)

with r(t) = t.bfloat16().to(t.dtype) (RNE) and everything accumulated in the tensors' own dtype (fp32 or float64).  The
1x1 head `cm.conv6` and everything that is not a convolution stay as the oracle has them.  With `rounding=False`
the substituted function only forwards, so the result must be the oracle's own: tests/test_fusat_bf16_cpu.py pins
that against tests/golden/fusat_b4.npz.
"""
import contextlib

import torch
import torch.nn.functional as F

from oracle import fusat_oracle as O


def rne_bf16(t):
    return t.bfloat16().to(t.dtype)


class RoundedConv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, pad):
        xr, wr = rne_bf16(x), rne_bf16(w)
        ctx.save_for_backward(xr, wr)
        ctx.pad = pad
        return F.conv2d(xr, wr, b, padding=pad)

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        dyr = rne_bf16(dy)
        dx = torch.nn.grad.conv2d_input(xr.shape, wr, dyr, padding=ctx.pad) if ctx.needs_input_grad[0] else None
        dw = torch.nn.grad.conv2d_weight(xr, wr.shape, dyr, padding=ctx.pad) if ctx.needs_input_grad[1] else None
        db = dy.sum(dim=(0, 2, 3)) if ctx.needs_input_grad[2] else None
        return dx, dw, db, None


def _conv2d(rounding):
    def conv2d(x, w, b=None, padding=0):
        if rounding and tuple(w.shape[2:]) == (3, 3):
            return RoundedConv3x3.apply(x, w, b, padding)
        return F.conv2d(x, w, b, padding=padding)

    return conv2d


class _Functional:
    """torch.nn.functional with conv2d replaced: every other name is looked up there"""

    def __init__(self, rounding):
        self.conv2d = _conv2d(rounding)

    def __getattr__(self, name):
        return getattr(F, name)


@contextlib.contextmanager
def substituted(rounding=True):
    """oracle.fusat_oracle with its convolution replaced (the module object itself is not edited on disk)"""
    orig, O.F = O.F, _Functional(rounding)
    try:
        yield
    finally:
        O.F = orig


def forward(sd, x1, x2, train=True, rounding=True):
    with substituted(rounding):
        return O.forward(sd, x1, x2, train=train)
