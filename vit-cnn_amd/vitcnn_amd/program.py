"""What every comparison model's hand-written program shares: the arrival-counter pool, the
`Program` base class (parameter pointer table, workspace, BatchNorm bookkeeping, dropout seeding, the backward's flat
gradient) and the one autograd bridge, `ProgramFunction`, with `run()`, the common tail of every model's `forward`.

A model file keeps its parameter tree, its shape checks and a `Program` subclass with the model-specific `_forward` and
`backward` bodies.  The unbatched `vc_gemm_ex` wrapper `gemm()`, the layer helpers built on it (`linear`, `dropped`,
`ln`, `bn_bwd`, ... and their backwards) and the pre-norm transformer encoder of MHST and GLT-Net (`encoder_fwd` /
`encoder_bwd`) are here too; only S2EFT keeps a `gemm()` of its own (`vc_gemm`: batch strides, a grouped mode, a side
stream).
"""
from __future__ import annotations

import functools

import torch

from . import seeds
from .flat import F32
from .model import N_COUNTERS

ATTN_HEADS, ATTN_DIM_HEAD = 4, 16   # vc_s2eft_attn_*: the encoder's attention

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

    def bytes(self, *shape):
        return torch.empty(*shape, dtype=torch.uint8, device=self.dev)

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

    def ln(self, pfx, X, R, ldx, D=None):
        """LayerNorm of R rows at X (ptr, ld ldx) of width D (the model width `self.D` if None) -> (Y [R, D], mean,
        rstd)"""
        D = D or self.D
        Y, mu, rs = self.new(R, D), self.new(R), self.new(R)
        self.L.vc_layernorm_fwd(R, D, X, ldx, self.P[pfx + ".weight"], self.P[pfx + ".bias"], self.LN_EPS, Y.data_ptr(),
                                D, mu.data_ptr(), rs.data_ptr(), self.s)
        return Y, mu, rs

    def gemm(self, tA, tB, M, N, K, A, lda, Bm, ldb, C, ldc, *, beta=0.0, bias=None, add=None, add_ld=0, add_mod=0,
             bias_grad=None):
        """C = op(A) op(B) + beta C (+ bias per column, + the row addend `add`, row i reading row i % add_mod of it if
        add_mod; bias_grad: the column sums of A^T's rows, a Linear's db): one unbatched `vc_gemm_ex` with the
        program's workspace, counters and stream"""
        self.L.vc_gemm_ex(tA, tB, M, N, K, 1.0, A, lda, 0, Bm, ldb, 0, beta, C, ldc, 0, 1, bias, add, add_ld, add_mod, 0,
                          bias_grad, self.scr.data_ptr(), self.SCRATCH, self.cnt, N_COUNTERS, self.s)

    def linear(self, x, M, K, N, pfx, bias=True, ldx=None, **kw):
        """y [M, N] = x W^T (+ b) of the Linear `pfx`; x a tensor or a pointer, its rows ldx (K) floats apart"""
        y = self.new(M, N)
        self.gemm(0, 1, M, N, K, x if isinstance(x, int) else x.data_ptr(), ldx or K, self.P[pfx + ".weight"], K,
                  y.data_ptr(), N, bias=self.P[pfx + ".bias"] if bias else None, **kw)
        return y

    def pack3x3(self, name, O, C):
        """the 3x3 conv weight `name` tap-major, Wt [O][9][C rounded up to 4] (repacked per forward: the parameters
        move)"""
        wt = self.new(O * 9 * ((C + 3) // 4 * 4))
        self.L.vc_conv3x3_pack(O, C, 0, self.P[name], wt.data_ptr(), 0.0, self.s)
        return wt

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

    def drop_p(self, mod):
        """the Dropout module's p in training, 0 in eval"""
        return float(mod.p) if self.train else 0.0

    def dropped(self, site, x, add, n, p, D):
        """add + dropout_p(x) over n floats in rows of D, as a new tensor (x + add, or x itself, at p = 0)"""
        if p > 0:
            y = torch.empty_like(x)
            self.drop(site, x, add, y, n, p)
            return y
        if add is None:
            return x
        y = torch.empty_like(x)
        self.L.vc_add2_2d(n // D, D, x.data_ptr(), D, add.data_ptr(), D, y.data_ptr(), D, 0.0, self.s)
        return y

    def drop_bwd(self, site, dy, n, p):
        if p <= 0:
            return dy
        dx = torch.empty_like(dy)
        self.L.vc_dropout_bwd(n, dy.data_ptr(), self.masks[site].data_ptr(), p, dx.data_ptr(), self.s)
        return dx

    # ------------------------------------------------------------ the pre-norm encoder (MHST, GLT-Net)
    def encoder_fwd(self, X, *, prefix, layers, T, D, hidden, ff, site):
        """A `Transformer` of pre-norm layers (x += drop(to_out(attn(LN x))); x += drop(W2 drop(gelu(W1 LN x)))) of 4
        heads of 16 over B x T tokens of width D, on S2EFT's attention kernels.  `prefix`: the parameters are
        `{prefix}.layers.{i}...`; `layers`: the nn.ModuleList the dropout probabilities are read from; `hidden`: the
        MLP's width; `ff`: the name of the feed-forward's nn.Sequential ("mlp" / "net"); the keep masks are saved under
        `{site}{i}.attn` / `.ff1` / `.ff2`.  -> (the output [B T, D], the layers' saved state for `encoder_bwd`)"""
        L, B = self.L, self.B
        H, dh = ATTN_HEADS, ATTN_DIM_HEAD
        R, E = B * T, H * dh
        saved = []
        for li, (att, mlp) in enumerate(layers):
            pre = f"{prefix}.layers.{li}"
            att, mlp = att.fn.fn, getattr(mlp.fn.fn, ff)
            pa, p1, p2 = self.drop_p(att.to_out[1]), self.drop_p(mlp[2]), self.drop_p(mlp[4])
            Y, mu, rs = self.ln(pre + ".0.fn.norm", X.data_ptr(), R, D, D)
            qkv = self.linear(Y, R, D, 3 * E, pre + ".0.fn.fn.to_qkv", bias=False)
            O, lse = self.new(R, E), self.new(B, H, T)
            L.vc_s2eft_attn_fwd(B, T, H, qkv.data_ptr(), dh ** -0.5, O.data_ptr(), lse.data_ptr(), self.s)
            A2 = self.linear(O, R, E, D, pre + ".0.fn.fn.to_out.0")
            X2 = self.dropped(f"{site}{li}.attn", A2, X, R * D, pa, D)
            Y2, mu2, rs2 = self.ln(pre + ".1.fn.norm", X2.data_ptr(), R, D, D)
            H1 = self.linear(Y2, R, D, hidden, f"{pre}.1.fn.fn.{ff}.0")
            Gl = self.new(R, hidden)
            L.vc_gelu_fwd(R * hidden, H1.data_ptr(), Gl.data_ptr(), self.s)
            Gd = self.dropped(f"{site}{li}.ff1", Gl, None, R * hidden, p1, hidden)
            F2 = self.linear(Gd, R, hidden, D, f"{pre}.1.fn.fn.{ff}.3")
            X3 = self.dropped(f"{site}{li}.ff2", F2, X2, R * D, p2, D)
            saved.append(dict(X=X, Y=Y, mu=mu, rs=rs, qkv=qkv, O=O, lse=lse, X2=X2, Y2=Y2, mu2=mu2, rs2=rs2, H1=H1, Gd=Gd,
                              pa=pa, p1=p1, p2=p2))
            X = X3
        return X, saved

    def encoder_bwd(self, dX, saved, *, prefix, T, D, hidden, ff, site):
        """`encoder_fwd` backwards: the layers' parameter gradients into the flat gradient -> the input's gradient"""
        L, B = self.L, self.B
        H, dh = ATTN_HEADS, ATTN_DIM_HEAD
        R, E = B * T, H * dh
        for li in reversed(range(len(saved))):
            pre = f"{prefix}.layers.{li}"
            st = saved[li]
            dF2 = self.drop_bwd(f"{site}{li}.ff2", dX, R * D, st["p2"])
            dGd = self.linear_bwd(dF2, st["Gd"], R, hidden, D, f"{pre}.1.fn.fn.{ff}.3")
            dGl = self.drop_bwd(f"{site}{li}.ff1", dGd, R * hidden, st["p1"])
            dH1 = self.new(R, hidden)
            L.vc_gelu_bwd(R * hidden, dGl.data_ptr(), st["H1"].data_ptr(), dH1.data_ptr(), self.s)
            dY2 = self.linear_bwd(dH1, st["Y2"], R, D, hidden, f"{pre}.1.fn.fn.{ff}.0")
            dX2 = self.new(R, D)   # the residual's share, then LN's added to it
            L.vc_add2_2d(R, D, dX.data_ptr(), D, None, 0, dX2.data_ptr(), D, 0.0, self.s)
            self.ln_bwd(pre + ".1.fn.norm", dY2, st["X2"].data_ptr(), D, st["mu2"], st["rs2"], R, D, dX2.data_ptr(), D, 1.0)
            dA2 = self.drop_bwd(f"{site}{li}.attn", dX2, R * D, st["pa"])
            dO = self.linear_bwd(dA2, st["O"], R, E, D, pre + ".0.fn.fn.to_out.0")
            dqkv = self.new(R, 3 * E)
            L.vc_s2eft_attn_bwd(B, T, H, st["qkv"].data_ptr(), st["O"].data_ptr(), dO.data_ptr(), st["lse"].data_ptr(),
                                dh ** -0.5, dqkv.data_ptr(), self.s)
            dY = self.linear_bwd(dqkv, st["Y"], R, D, 3 * E, pre + ".0.fn.fn.to_qkv", bias=False)
            dXi = self.new(R, D)
            L.vc_add2_2d(R, D, dX2.data_ptr(), D, None, 0, dXi.data_ptr(), D, 0.0, self.s)
            self.ln_bwd(pre + ".0.fn.norm", dY, st["X"].data_ptr(), D, st["mu"], st["rs"], R, D, dXi.data_ptr(), D, 1.0)
            dX = dXi
        return dX

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

    def linear_bwd(self, dy, x, M, K, N, pfx, bias=True, need_dx=True, dx=None, lddx=None, beta=0.0, ldx=None):
        """dW (+ db) of y = x W^T + b into the flat gradient; then dx = dy W: a new [M, K] tensor, returned, or
        beta dx + dy W at the pointer `dx` (ld lddx), or with need_dx=False neither allocated nor launched"""
        self.gemm(1, 0, N, K, M, dy.data_ptr(), N, x if isinstance(x, int) else x.data_ptr(), ldx or K,
                  self.G[pfx + ".weight"], K, bias_grad=self.G[pfx + ".bias"] if bias else None)
        if not need_dx:
            return None
        out = None
        if dx is None:
            out = self.new(M, K)
            dx, lddx = out.data_ptr(), K
        self.gemm(0, 0, M, K, N, dy.data_ptr(), N, self.P[pfx + ".weight"], K, dx, lddx, beta=beta)
        return out

    def ln_bwd(self, pfx, dY, X, ldx, mu, rs, R, D, dx, lddx, beta):
        """LayerNorm `pfx` backwards over R rows of width D: dx (ptr, ld lddx) = beta dx + ..., dgamma and dbeta into
        the flat gradient"""
        self.L.vc_layernorm_bwd(R, D, dY.data_ptr(), D, X, ldx, self.P[pfx + ".weight"], mu.data_ptr(), rs.data_ptr(),
                                dx, lddx, beta, self.G[pfx + ".weight"], self.G[pfx + ".bias"], 0.0, self.scr.data_ptr(),
                                self.SCRATCH, self.s)

    def bn_bwd(self, pfx, dz, y, mean, inv, M, C, beta_w=0.0):
        """BatchNorm + ReLU backwards -> dy [M, C]; dgamma, dbeta = beta_w (theirs) + this application's"""
        dy = self.new(M, C)
        self.L.vc_bn_bwd_relu_ex(1 if self.train else 0, M, C, dz.data_ptr(), C, y.data_ptr(), C, mean.data_ptr(),
                                 inv.data_ptr(), self.P[pfx + ".weight"], self.P[pfx + ".bias"], dy.data_ptr(), C, 0.0,
                                 self.G[pfx + ".weight"], self.G[pfx + ".bias"], beta_w, self.scr.data_ptr(),
                                 self.SCRATCH, self.cnt, N_COUNTERS, self.s)
        return dy

    def reduce_part(self, part, width, col, n, out):
        """out[0:n] = sum over the samples of part[b][col : col + n] (fixed order)"""
        self.L.vc_colsum(self.B, n, part.data_ptr() + F32 * col, width, out, 0.0, self.scr.data_ptr(), self.SCRATCH,
                         self.s)

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
