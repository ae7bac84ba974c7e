"""What every comparison model's hand-written program shares: the arrival-counter pool, the
`Program` base class (parameter pointer table, workspace, BatchNorm bookkeeping, dropout seeding, the backward's flat
gradient) and the one autograd bridge, `ProgramFunction`, with `run()`, the common tail of every model's `forward`.

A model file keeps its parameter tree, its shape checks and a `Program` subclass with the model-specific `_forward` and
`backward` bodies and its own `gemm()` wrapper (the wrappers differ in beta, addends and batch strides; only their tail
`scr, SCRATCH, cnt, N_COUNTERS, s` is common).
"""
from __future__ import annotations

import functools

import torch

from . import seeds
from .flat import F32
from .model import N_COUNTERS

BN_MOMENTUM = 0.1
_COUNTER_BUFS = {}


def counters(dev, stream):
    """one zeroed arrival-counter array per (device, stream) (split-K in-launch combine, BN
    reductions): kernels of one stream run in order and each leaves its counters zero"""
    key = (dev.type, dev.index, stream)
    if key not in _COUNTER_BUFS:
        _COUNTER_BUFS[key] = torch.zeros(N_COUNTERS, dtype=torch.int32, device=dev)
    return _COUNTER_BUFS[key].data_ptr()


class Program:
    """One forward (saving what the backward reads) and its hand-written backward, all on the current stream.
    Subclasses set NAME (the model's name in messages), pass their module's `lib()` up and define `_forward()` and
    `backward(*grads)`."""

    NAME = ""
    COUNTERS = True     # S2EFT's GEMMs (vc_gemm) take no arrival counters
    LN_EPS = 1e-5       # nn.LayerNorm's default

    def __init__(self, L, m, needs_grad, *xs):
        self.m, self.L, self.dev = m, L, xs[0].device
        self.needs_grad = needs_grad
        self.s = torch.cuda.current_stream(self.dev).cuda_stream
        self.B = xs[0].shape[0]
        self.cnt = counters(self.dev, self.s) if self.COUNTERS else None
        self.train = m.training
        self.nbt = []

    @functools.cached_property
    def P(self):
        """the parameter pointer table, built at its first use in the forward (FusAtNet's tape reads the modules)"""
        base = self.m._flat_store.data_ptr()
        return {n: base + F32 * o for n, o in self.m._poff.items()}

    def new(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.dev)

    def scratch(self, floats, grow=False):
        """the fp32 workspace (split-K slabs, fixed-order partial sums), cached on the model per device so that a
        forward allocates nothing: `self.scr`, and its size `self.SCRATCH` as the kernels are told it (the split-K plan
        depends on it).  One buffer is kept: of exactly `floats`, or (grow) the largest asked for so far."""
        cache = self.m.__dict__.setdefault("_vc_scratch", {})
        key = str(self.dev)
        buf = cache.get(key)
        if buf is None or (buf.numel() < floats if grow else buf.numel() != floats):
            cache.clear()
            buf = cache[key] = torch.empty(floats, dtype=torch.float32, device=self.dev)
        self.scr, self.SCRATCH = buf, buf.numel()

    # ------------------------------------------------------------ forward
    def forward(self):
        self.nbt = []
        out = self._forward()
        self.count_batches()
        return out

    def count_batches(self):
        if self.nbt:   # every executed BatchNorm's num_batches_tracked += 1: one multi-tensor launch
            torch._foreach_add_(self.nbt, 1)

    def bn_momentum(self, mod):
        """the BatchNorm's momentum; in training the module is also noted for `count_batches`"""
        if self.train:
            self.nbt.append(mod.num_batches_tracked)
        return mod.momentum if mod.momentum is not None else BN_MOMENTUM

    def bn(self, pfx, mod, y, M, C, relu=1):
        """train-mode (batch statistics, running statistics updated) or eval-mode BatchNorm (+ ReLU) of rows y"""
        mean, invstd, z = self.new(C), self.new(C), self.new(M, C)
        self.L.vc_bn_forward_ex(1 if self.train else 0, M, C, y.data_ptr(), C, mod.eps, self.bn_momentum(mod),
                                mean.data_ptr(), invstd.data_ptr(), mod.running_mean.data_ptr(),
                                mod.running_var.data_ptr(), self.P[pfx + ".weight"], self.P[pfx + ".bias"], relu,
                                z.data_ptr(), C, self.scr.data_ptr(), self.SCRATCH, self.cnt, N_COUNTERS, self.s)
        return z, mean, invstd

    def ln(self, pfx, X, R, ldx):
        """LayerNorm of R rows at X (ptr, ld ldx) of the model width `self.D` -> (Y [R, D], mean, rstd)"""
        D = self.D
        Y, mu, rs = self.new(R, D), self.new(R), self.new(R)
        self.L.vc_layernorm_fwd(R, D, X, ldx, self.P[pfx + ".weight"], self.P[pfx + ".bias"], self.LN_EPS, Y.data_ptr(),
                                D, mu.data_ptr(), rs.data_ptr(), self.s)
        return Y, mu, rs

    def rows(self, x, C, HW):
        """NCHW -> channels-last rows padded to a multiple of 4 floats (zero-filled)"""
        ld = (C + 3) // 4 * 4
        y = self.new(self.B * HW, ld)
        if ld == C:
            self.L.vc_nchw_to_nhwc(self.B, C, HW, x.data_ptr(), y.data_ptr(), self.s)
        else:
            self.L.vc_nchw_to_nhwc_pad(self.B, C, HW, x.data_ptr(), y.data_ptr(), ld, self.s)
        return y, ld

    # ------------------------------------------------------------ dropout
    def seed_dropout(self, active):
        """`active`: this forward draws masks.  Then the seed is the attached device-resident step seed (seeds.attach:
        nothing is drawn on the host, the _ds entry points read it there) or one host draw; site k of the forward
        uses seed + 1000003 k.  Every keep mask is kept as bytes in `self.masks`."""
        self.masks = {}
        self.dseed = seeds.state_for(self.m, self.dev) if active else None
        self.seed = seeds.host_seed() if active and self.dseed is None else 0

    def drop(self, site, x, add, y, n, p):
        """y = add + dropout_p(x) (add may be None, y may be x); the keep mask is saved under `site`"""
        mk = torch.empty(n, dtype=torch.uint8, device=self.dev)
        if self.dseed is not None:
            self.L.vc_dropout_fwd_ds(n, x.data_ptr(), add.data_ptr() if add is not None else None, y.data_ptr(),
                                     mk.data_ptr(), p, self.dseed.cur_ptr, seeds.SITE_STRIDE * len(self.masks), self.s)
        else:
            self.L.vc_dropout_fwd(n, x.data_ptr(), add.data_ptr() if add is not None else None, y.data_ptr(),
                                  mk.data_ptr(), p, (self.seed + seeds.SITE_STRIDE * len(self.masks)) % (1 << 63),
                                  self.s)
        self.masks[site] = mk

    # ------------------------------------------------------------ backward
    def new_grad(self):
        """the zero-filled flat gradient (the backward overwrites each parameter's slice once; the alignment gaps and
        what the forward never reaches stay zero) and `self.G`, its pointer table"""
        m = self.m
        grad = self.new(m._n_params)
        self.L.vc_fill(m._n_params, grad.data_ptr(), 0.0, self.s)
        gb = grad.data_ptr()
        self.G = {n: gb + F32 * o for n, o in m._poff.items()}
        return grad

    def prepare_grads(self, grads):
        """the incoming output gradients as `backward`'s arguments: contiguous fp32"""
        return [g.detach().to(torch.float32).contiguous() for g in grads]


class ProgramFunction(torch.autograd.Function):
    """The autograd bridge of every comparison model: the forward runs a new `program(model, needs_grad, *inputs)`
    and keeps it for the backward only if one can follow; the backward returns the flat buffer's gradient."""

    @staticmethod
    def forward(ctx, model, flat, needs_grad, program, *xs):
        prog = program(model, needs_grad, *xs)
        out = prog.forward()
        ctx.model_name, ctx.n_in = prog.NAME, len(xs)
        ctx.prog = prog if needs_grad else None
        return out

    @staticmethod
    def backward(ctx, *grads):
        prog, ctx.prog = ctx.prog, None
        if prog is None:
            raise RuntimeError(f"{ctx.model_name}: backward through a forward run without grad")
        grad = prog.backward(*prog.prepare_grads(grads))
        return (None, grad, None, None) + (None,) * ctx.n_in


def run(model, program, *xs):
    """the tail of a model's forward, behind its own shape checks: the flat buffer made current, then `program` run
    over the inputs through the bridge"""
    model._ensure_flat()
    if model._flat_store.device != xs[0].device:
        raise RuntimeError(f"model and input{'s' if len(xs) > 1 else ''} are on different devices")
    needs_grad = torch.is_grad_enabled() and model._flat_store.requires_grad
    return ProgramFunction.apply(model, model._flat_store, needs_grad, program, *xs)
