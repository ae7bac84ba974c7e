"""EndNet comparison model (per-pixel encoder-decoder fusion network) on the MI355X path.

Reference: `model/compare_method/EndNet.py` (class `EndNet` :9-90), built by `model_utils.py:119-128` (patch 1, Adam lr
1e-3, `EndNet_Loss`).  The module keeps the reference's parameter tree, creation order and default initialisers, so
`state_dict()` has the reference's 93 keys, `.pth` files interchange and the same `torch.manual_seed` draws the same
initial values.  `joint_encoder_bn7` is declared and never applied, as in the reference (:46, :76): its affine gets a
zero gradient and stays bit-unchanged, its running statistics and `num_batches_tracked` never move.

Forward and backward are one hand-written program over pixel rows [B, C]; the parameters live in
one flat fp32 buffer whose `.grad` the backward fills.  Each of the 19 Linear layers is ONE launch forward
(`vc_fc_fused_fwd`: Linear + BatchNorm1d + ReLU with the batch statistics and the running-statistics update inside,
Linear + sigmoid for the decoders, plain Linear for `joint_encoder_fc7`) and one launch backward (`vc_fc_fused_bwd`:
mask, BatchNorm sums, dz, dW, db, dgamma, dbeta) plus a `vc_gemm_ex` for the data gradient dz W where a layer has one
(the two first layers' inputs are data).  `cat([x1, x2], 1)` costs nothing: `encoder_fc4_a` / `_b` write the two
halves of one [B, 256] buffer, and their backward reads the halves of its gradient.

Deviations: train mode needs 2 <= B <= 1024 (`ValueError`; torch's BatchNorm1d raises at B = 1 too, 1024 is the fused
layer's LDS bound), eval takes any B >= 1; the constructor refuses band / class counts outside the tested envelope.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import program
from ._lib import lib
from .flat import F32, FlatParams

FILTERS = (16, 32, 64, 128)
C_MAX, NCLS_MAX = 512, 64           # bands per modality (the fused layer's K bound), classes
TRAIN_B_MAX = 1024                  # VC_FC_TRAIN_BMAX (include/vitcnn.h)
FC_PLAIN, FC_BN_RELU, FC_SIGMOID = 0, 1, 2


class EndNet(FlatParams, nn.Module):
    """Same constructor as the reference class; forward(x1 [B, C1] or [B, C1, 1, 1], x2 likewise) ->
    (out [B, n_classes], de_x1 [B, C1], de_x2 [B, C2], x1 [B, C1], x2 [B, C2]), in train and in eval."""

    def __init__(self, input_channels, input_channels2, n_classes):
        super().__init__()
        if not 1 <= input_channels <= C_MAX:
            raise ValueError(f"EndNet MI355X path: 1..{C_MAX} HSI bands, got {input_channels}")
        if not 1 <= input_channels2 <= C_MAX:
            raise ValueError(f"EndNet MI355X path: 1..{C_MAX} LiDAR bands, got {input_channels2}")
        if not 2 <= n_classes <= NCLS_MAX:
            raise ValueError(f"EndNet MI355X path: 2..{NCLS_MAX} classes, got {n_classes}")
        self.C1, self.C2, self.ncls = input_channels, input_channels2, n_classes
        f = FILTERS
        self.activation = nn.ReLU(inplace=True)
        self.sigmoid = nn.Sigmoid()
        # creation order = the reference's (:22-57)
        for sfx, cin in (("_a", input_channels), ("_b", input_channels2)):
            for i, (k, n) in enumerate(((cin, f[0]), (f[0], f[1]), (f[1], f[2]), (f[2], f[3])), 1):
                setattr(self, f"encoder_fc{i}{sfx}", nn.Linear(k, n))
                setattr(self, f"encoder_bn{i}{sfx}", nn.BatchNorm1d(n))
        self.joint_encoder_fc5 = nn.Linear(f[3] * 2, f[3])
        self.joint_encoder_bn5 = nn.BatchNorm1d(f[3])
        self.joint_encoder_fc6 = nn.Linear(f[3], f[2])
        self.joint_encoder_bn6 = nn.BatchNorm1d(f[2])
        self.joint_encoder_fc7 = nn.Linear(f[2], n_classes)
        self.joint_encoder_bn7 = nn.BatchNorm1d(n_classes)
        for sfx, cout in (("_a", input_channels), ("_b", input_channels2)):
            for i, (k, n) in enumerate(((f[3], f[2]), (f[2], f[1]), (f[1], f[0]), (f[0], cout)), 1):
                setattr(self, f"decoder_fc{i}{sfx}", nn.Linear(k, n))
        self._build_flat()

    def forward(self, x1: torch.Tensor, x2: torch.Tensor):
        dev_ok = x1.device.type == "cuda" and x2.device.type == "cuda"
        x1, x2 = _pixel_rows(x1, self.C1, "x1"), _pixel_rows(x2, self.C2, "x2")
        if x1.shape[0] != x2.shape[0] or x1.shape[0] < 1:
            raise RuntimeError(f"x1 and x2 need the same batch size >= 1: {x1.shape[0]} / {x2.shape[0]}")
        B = x1.shape[0]
        if self.training and B < 2:    # torch's BatchNorm1d message
            raise ValueError(f"Expected more than 1 value per channel when training, got input size [{B}, {self.C1}]")
        if self.training and B > TRAIN_B_MAX:
            raise ValueError(f"EndNet MI355X path: train mode takes at most {TRAIN_B_MAX} rows per batch (the fused "
                             f"Linear + BatchNorm1d layer keeps the batch in LDS), got {B}")
        if not dev_ok:
            raise RuntimeError("EndNet MI355X path: inputs must be on a ROCm (cuda) device; no CPU fallback")
        out, de1, de2 = program.run(self, _Program, x1, x2)
        return out, de1, de2, x1, x2


def _pixel_rows(x, C, name):
    """[B, C] or [B, C, 1, 1] (what PatchBatcher / SlidingWindowInference yield at patch_size 1: the same memory) as
    contiguous fp32 rows [B, C]"""
    if x.dim() == 4 and x.shape[2] == 1 and x.shape[3] == 1:
        x = x.reshape(x.shape[0], x.shape[1])
    if x.dim() != 2 or x.shape[1] != C:
        raise RuntimeError(f"expected {name} [B, {C}] or [B, {C}, 1, 1], got {list(x.shape)}")
    return x.detach().to(torch.float32).contiguous()


class _Program(program.Program):
    NAME = "EndNet"

    def __init__(self, m: EndNet, needs_grad, x1, x2):
        super().__init__(lib(), m, needs_grad, x1, x2)
        self.x1, self.x2 = x1, x2
        self.scratch(1 << 22)   # fp32 workspace of the data-gradient GEMMs (split-K slabs)
        self.mods = dict(m.named_children())

    def prepare_grads(self, grads):
        """(dout, dde1, dde2); the gradient of an output the loss did not use is zero"""
        if self.B > TRAIN_B_MAX:
            raise RuntimeError(f"EndNet MI355X path: the backward takes at most {TRAIN_B_MAX} rows, got {self.B}")
        m = self.m
        return [torch.zeros(self.B, n, dtype=torch.float32, device=self.dev) if d is None
                else d.detach().to(torch.float32).contiguous() for d, n in zip(grads, (m.ncls, m.C1, m.C2))]

    # ------------------------------------------------------------ one layer
    def fc(self, name, bn, mode, x, ldx, K, N, y=None, ldy=None):
        """y (ptr, ld ldy; a new [B, N] buffer by default) = act(norm(x W^T + b)) in one launch; returns the record the
        backward reads"""
        B = self.B
        buf = None
        if y is None:
            buf = self.new(B, N)
            y, ldy = buf.data_ptr(), N
        rec = dict(name=name, bn=bn, mode=mode, x=x, ldx=ldx, K=K, N=N, y=y, ldy=ldy, buf=buf)
        P = self.P
        if mode == FC_BN_RELU:
            mod = self.mods[bn]
            mom = self.bn_momentum(mod)
            xhat = st0 = st1 = None
            if self.train or self.needs_grad:   # what the backward reads (the train-mode kernel always writes it);
                rec["xhat"], rec["st"] = self.new(B, N), self.new(2, N)   # eval with no backward to follow: nothing
                xhat, st0, st1 = rec["xhat"].data_ptr(), rec["st"][0].data_ptr(), rec["st"][1].data_ptr()
            self.L.vc_fc_fused_fwd(mode, 1 if self.train else 0, B, K, N, x, ldx, P[name + ".weight"], P[name + ".bias"],
                                   P[bn + ".weight"], P[bn + ".bias"], mod.running_mean.data_ptr(),
                                   mod.running_var.data_ptr(), mod.eps, mom, y, ldy, xhat, st0, st1, self.s)
        else:
            self.L.vc_fc_fused_fwd(mode, 0, B, K, N, x, ldx, P[name + ".weight"], P[name + ".bias"], None, None, None,
                                   None, 0.0, 0.0, y, ldy, None, None, None, self.s)
        return rec

    def fc_bwd(self, rec, dy, lddy, dx=None, lddx=0, beta=0.0):
        """the layer's parameter gradients (overwritten) in one launch and, with dx (ptr), dx = beta dx + dz W"""
        B, K, N, name, bn = self.B, rec["K"], rec["N"], rec["name"], rec["bn"]
        G, P = self.G, self.P
        dz = self.new(B, N) if dx is not None else None
        isbn = rec["mode"] == FC_BN_RELU
        self.L.vc_fc_fused_bwd(rec["mode"], 1 if self.train else 0, B, K, N, dy, lddy, rec["y"], rec["ldy"],
                               rec["xhat"].data_ptr() if isbn else None, rec["x"], rec["ldx"],
                               P[bn + ".weight"] if isbn else None, rec["st"][1].data_ptr() if isbn else None,
                               dz.data_ptr() if dz is not None else None, N, G[name + ".weight"], G[name + ".bias"],
                               G[bn + ".weight"] if isbn else None, G[bn + ".bias"] if isbn else None, self.s)
        if dx is not None:
            self.gemm(0, 0, B, K, N, dz.data_ptr(), N, P[name + ".weight"], K, dx, lddx, beta=beta)

    # ------------------------------------------------------------ forward
    def _forward(self):
        m, f = self.m, FILTERS
        joint = self.joint = self.new(self.B, 2 * f[3])      # cat([x1, x2], 1): the branches write its halves
        self.enc = {}
        for sfx, x, cin, half in (("_a", self.x1, m.C1, 0), ("_b", self.x2, m.C2, 1)):
            recs, ptr, ld = [], x.data_ptr(), cin
            for i, (k, n) in enumerate(((cin, f[0]), (f[0], f[1]), (f[1], f[2]), (f[2], f[3])), 1):
                last = i == 4
                r = self.fc(f"encoder_fc{i}{sfx}", f"encoder_bn{i}{sfx}", FC_BN_RELU, ptr, ld, k, n,
                            joint.data_ptr() + F32 * half * f[3] if last else None, 2 * f[3] if last else None)
                recs.append(r)
                ptr, ld = r["y"], r["ldy"]
            self.enc[sfx] = recs
        self.r5 = self.fc("joint_encoder_fc5", "joint_encoder_bn5", FC_BN_RELU, joint.data_ptr(), 2 * f[3], 2 * f[3], f[3])
        self.r6 = self.fc("joint_encoder_fc6", "joint_encoder_bn6", FC_BN_RELU, self.r5["y"], f[3], f[3], f[2])
        self.r7 = self.fc("joint_encoder_fc7", None, FC_PLAIN, self.r6["y"], f[2], f[2], m.ncls)
        self.dec = {}
        for sfx, cout in (("_a", m.C1), ("_b", m.C2)):
            recs, ptr, ld = [], self.r5["y"], f[3]
            for i, (k, n) in enumerate(((f[3], f[2]), (f[2], f[1]), (f[1], f[0]), (f[0], cout)), 1):
                r = self.fc(f"decoder_fc{i}{sfx}", None, FC_SIGMOID, ptr, ld, k, n)
                recs.append(r)
                ptr, ld = r["y"], r["ldy"]
            self.dec[sfx] = recs
        return self.r7["buf"], self.dec["_a"][-1]["buf"], self.dec["_b"][-1]["buf"]

    # ------------------------------------------------------------ backward
    def backward(self, dout, dde1, dde2):
        """the flat gradient of every parameter; each is written once (overwritten), the alignment gaps and the
        never-applied joint_encoder_bn7 stay zero"""
        m, f, B = self.m, FILTERS, self.B
        grad = self.new_grad()
        d6 = self.new(B, f[2])
        self.fc_bwd(self.r7, dout.data_ptr(), m.ncls, d6.data_ptr(), f[2])
        d5 = self.new(B, f[3])          # joint_x feeds fc6 and both decoders: the first writes, the others add
        self.fc_bwd(self.r6, d6.data_ptr(), f[2], d5.data_ptr(), f[3])
        for sfx, dde, cout in (("_a", dde1, m.C1), ("_b", dde2, m.C2)):
            dy, ld = dde.data_ptr(), cout
            keep = [dde]
            for r in reversed(self.dec[sfx]):
                first = r is self.dec[sfx][0]
                dxb = None if first else self.new(B, r["K"])
                self.fc_bwd(r, dy, ld, d5.data_ptr() if first else dxb.data_ptr(), r["K"], beta=1.0 if first else 0.0)
                if not first:
                    keep.append(dxb)
                    dy, ld = dxb.data_ptr(), r["K"]
        dj = self.new(B, 2 * f[3])
        self.fc_bwd(self.r5, d5.data_ptr(), f[3], dj.data_ptr(), 2 * f[3])
        for sfx, half in (("_a", 0), ("_b", 1)):
            dy, ld = dj.data_ptr() + F32 * half * f[3], 2 * f[3]
            for r in reversed(self.enc[sfx]):
                first = r is self.enc[sfx][0]          # its input is data: no data gradient
                dxb = None if first else self.new(B, r["K"])
                self.fc_bwd(r, dy, ld, None if first else dxb.data_ptr(), r["K"])
                if not first:
                    keep.append(dxb)      # a buffer stays allocated while the next layer reads it
                    dy, ld = dxb.data_ptr(), r["K"]
        self.enc = self.dec = self.r5 = self.r6 = self.r7 = self.joint = None
        return grad
