"""MDL-RS comparison models ("More Diverse Means Better": early, middle, late and cross fusion CNNs) on the MI355X path.

Reference: `model/compare_method/DML_Hong.py` (`Early_fusion_CNN` :9-63, `Middle_fusion_CNN` :65-140,
`Late_fusion_CNN` :142-224, `Cross_fusion_CNN` :226-323), built by `model_utils.py:69-108` (patch 7, Adam lr 1e-3).
The modules keep the reference's parameter trees, creation order and initialisers (kaiming_normal_ fan_out for the
conv weights, torch's default conv bias, BatchNorm weight 1 / bias 0), so `state_dict()` has the reference's 44 /
72 / 86 / 72 keys, `.pth` files interchange and the same `torch.manual_seed` draws the same initial values.

Forward and backward are one hand-written program of HIP kernels over channels-last rows;
the parameters live in one flat fp32 buffer whose `.grad` the backward fills.  Every net is made of three stages:

* A: conv1 (3x3, `vc_conv3x3_tap_*`) - bn1 - ReLU - conv2 (1x1, `vc_gemm_ex`) - bn2 - ReLU - pool - conv3 - bn3 - ReLU;
* B: conv4 (1x1) - bn4 - ReLU - pool;
* C: conv5 (1x1) - bn5 - ReLU - conv6 (1x1) - bn6 - ReLU, then the average-pool head (`vc_avgpool_head_*`).

A BatchNorm in front of a pool is statistics only (`vc_bn_stats_ex`); its apply, the ReLU and the padded max pool
are one pass (`vc_maxpool2p_fwd`), and the pool's backward folds the ReLU mask in.  The layers Cross_fusion_CNN
shares between branches run once over the applications' stacked rows (2 M rows for conv4_a / conv4_b, 3 M for conv5 /
conv6: one GEMM forward, one per gradient), with BatchNorm per segment in the reference's order, so the running
statistics see the reference's sequence of updates and the parameter gradients are sums in a fixed order.

Deviation: the reference ends in `torch.squeeze`, which returns [n_classes] at B = 1; this path returns
[B, n_classes] for every B (Cross_fusion_CNN: a tuple of three such tensors, in train and in eval).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import program
from ._lib import lib
from .flat import F32, FlatParams
from .model import N_COUNTERS

FILTERS = (16, 32, 64, 128)     # n1 = 16: conv1, conv2, conv3 (= conv6), conv4 (= conv5) output widths
P_MIN, P_MAX = 3, 32            # a 3x3 conv needs a 3x3 map; the pooled maps of larger patches are untested
C1_MAX, C2_MAX, NCLS_MAX = 512, 8, 64   # the envelope the tests cover


def _check_supported(name, input_channels, input_channels2, n_classes, patch_size=None):
    """reject what a kernel cannot take, at construction"""
    if not 1 <= input_channels <= C1_MAX:
        raise ValueError(f"{name} MI355X path: 1..{C1_MAX} HSI bands, got {input_channels}")
    if not 1 <= input_channels2 <= C2_MAX:
        raise ValueError(f"{name} MI355X path: 1..{C2_MAX} LiDAR bands, got {input_channels2}")
    if not 2 <= n_classes <= NCLS_MAX:
        raise ValueError(f"{name} MI355X path: 2..{NCLS_MAX} classes, got {n_classes}")
    if patch_size is not None and not P_MIN <= patch_size <= P_MAX:
        raise ValueError(f"{name} MI355X path: patch_size must be in {P_MIN}..{P_MAX}, got {patch_size}")


def _branch(m, sfx, cin, upto):
    """conv1 .. conv<upto> with their BatchNorms under the reference's names (creation order = the reference's)"""
    f = FILTERS
    setattr(m, "conv1" + sfx, nn.Conv2d(cin, f[0], kernel_size=3, padding=1, bias=True))
    setattr(m, "bn1" + sfx, nn.BatchNorm2d(f[0]))
    setattr(m, "conv2" + sfx, nn.Conv2d(f[0], f[1], (1, 1)))
    setattr(m, "bn2" + sfx, nn.BatchNorm2d(f[1]))
    setattr(m, "conv3" + sfx, nn.Conv2d(f[1], f[2], kernel_size=3, padding=1, bias=True))
    setattr(m, "bn3" + sfx, nn.BatchNorm2d(f[2]))
    setattr(m, "conv4" + sfx, nn.Conv2d(f[2], f[3], (1, 1)))
    setattr(m, "bn4" + sfx, nn.BatchNorm2d(f[3]))
    if upto >= 6:
        _tail(m, sfx, f[3])


def _tail(m, sfx, cin):
    f = FILTERS
    setattr(m, "conv5" + sfx, nn.Conv2d(cin, f[3], (1, 1)))
    setattr(m, "bn5" + sfx, nn.BatchNorm2d(f[3]))
    setattr(m, "conv6" + sfx, nn.Conv2d(f[3], f[2], (1, 1)))
    setattr(m, "bn6" + sfx, nn.BatchNorm2d(f[2]))


class _MDLRS(FlatParams, nn.Module):
    """Same constructor as the reference classes: (input_channels, input_channels2, n_classes), plus an optional
    `patch_size` that is only checked (get_model passes it, so an unsupported patch fails at construction);
    forward(x1 [B,C1,P,P], x2 [B,C2,P,P]) -> logits [B, n_classes] (Cross_fusion_CNN: a tuple of three)."""

    def __init__(self, input_channels, input_channels2, n_classes, patch_size=None):
        super().__init__()
        _check_supported(type(self).__name__, input_channels, input_channels2, n_classes, patch_size)
        self.C1, self.C2, self.ncls = input_channels, input_channels2, n_classes
        self.activation = nn.ReLU(inplace=True)
        self.max_pool = nn.MaxPool2d(kernel_size=2, stride=2, padding=1)
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self._layers()
        for m in self.modules():   # weight_init of the reference (:40-46)
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self._build_flat()

    def forward(self, x1: torch.Tensor, x2: torch.Tensor):
        name = type(self).__name__
        if x1.device.type != "cuda" or x2.device.type != "cuda":
            raise RuntimeError(f"{name} MI355X path: inputs must be on a ROCm (cuda) device; no CPU fallback")
        if x1.dim() != 4 or x1.shape[1] != self.C1 or x1.shape[2] != x1.shape[3]:
            raise RuntimeError(f"expected x1 [B, {self.C1}, P, P], got {list(x1.shape)}")
        if x2.dim() != 4 or x2.shape[1] != self.C2 or x2.shape[0] != x1.shape[0] or x2.shape[2:] != x1.shape[2:]:
            raise RuntimeError(f"expected x2 [B, {self.C2}, P, P] matching x1, got {list(x2.shape)}")
        if not P_MIN <= x1.shape[2] <= P_MAX:
            raise RuntimeError(f"{name} MI355X path: patch_size must be in {P_MIN}..{P_MAX}, got {x1.shape[2]}")
        x1 = x1.detach().to(torch.float32).contiguous()
        x2 = x2.detach().to(torch.float32).contiguous()
        out = program.run(self, _Program, x1, x2)
        return out if self.KIND == "cross" else out[0]


class Early_fusion_CNN(_MDLRS):
    KIND = "early"

    def _layers(self):
        _branch(self, "", self.C1 + self.C2, 6)
        self.conv7 = nn.Conv2d(FILTERS[2], self.ncls, (1, 1))


def _two_branch_layers(m):
    """Middle_fusion_CNN's and Cross_fusion_CNN's tree: two branches up to conv4, one conv5 .. conv7"""
    _branch(m, "_a", m.C1, 4)
    _branch(m, "_b", m.C2, 4)
    _tail(m, "", 2 * FILTERS[3])
    m.conv7 = nn.Conv2d(FILTERS[2], m.ncls, (1, 1))


class Middle_fusion_CNN(_MDLRS):
    KIND = "middle"
    _layers = _two_branch_layers


class Late_fusion_CNN(_MDLRS):
    KIND = "late"

    def _layers(self):
        _branch(self, "_a", self.C1, 6)
        _branch(self, "_b", self.C2, 6)
        self.conv7 = nn.Conv2d(2 * FILTERS[2], self.ncls, (1, 1))


class Cross_fusion_CNN(_MDLRS):
    KIND = "cross"
    _layers = _two_branch_layers


class _Program(program.Program):
    NAME = "MDL-RS"

    def __init__(self, m: _MDLRS, needs_grad, x1, x2):
        super().__init__(lib(), m, needs_grad, x1, x2)
        self.x1, self.x2 = x1, x2
        self.Pp = x1.shape[2]
        self.scratch(1 << 22)   # fp32 workspace: split-K slabs, BatchNorm / conv partial sums
        self.mods = dict(m.named_children())
        self.H2 = self.Pp // 2 + 1     # after the first pool
        self.H3 = self.H2 // 2 + 1     # after the second

    def prepare_grads(self, dlogits):
        """[G, B, ncls] in one buffer; the gradient of an output the loss did not use is zero"""
        B, ncls = self.B, self.m.ncls
        ds = [torch.zeros(B, ncls, dtype=torch.float32, device=self.dev) if d is None
              else d.detach().to(torch.float32).contiguous() for d in dlogits]
        step, base = B * ncls * F32, ds[0].untyped_storage().data_ptr()
        if all(d.data_ptr() == ds[0].data_ptr() + i * step and d.untyped_storage().data_ptr() == base
               for i, d in enumerate(ds)):
            return [ds[0]]      # side by side in one buffer (Cross_fusion_CNN_Loss writes them so): no copy
        return [torch.stack(ds)]

    # ------------------------------------------------------------ primitives
    def conv1x1(self, name, x, M, K, N):
        """y [M, N] = x [M, K] W^T + bias"""
        y = self.new(M, N)
        self.gemm(0, 1, M, N, K, x, K, self.P[name + ".weight"], K, y.data_ptr(), N, bias=self.P[name + ".bias"])
        return y

    def conv1x1_bwd(self, name, x, dy, M, K, N, dx=None, beta=0.0):
        """dW, db (overwritten: one GEMM over all M rows) and, with dx, dx = beta dx + dy W"""
        self.gemm(1, 0, N, K, M, dy, N, x, K, self.G[name + ".weight"], K, bias_grad=self.G[name + ".bias"])
        if dx is not None:
            self.gemm(0, 0, M, K, N, dy, N, self.P[name + ".weight"], K, dx, K, beta=beta)

    def conv3x3(self, name, x, ldx, H, C, O):
        wt = self.pack3x3(name + ".weight", O, C)
        y = self.new(self.B * H * H, O)
        self.L.vc_conv3x3_tap_fwd(self.B, H, H, C, O, 1, x, ldx, wt.data_ptr(), self.P[name + ".bias"], y.data_ptr(), O,
                                  self.scr.data_ptr(), self.SCRATCH, self.s)
        return y, wt

    def conv3x3_wgrad(self, name, x, ldx, dy, H, C, O):
        self.L.vc_conv3x3_tap_wgrad_oihw(self.B, H, H, C, O, 1, x, ldx, dy, O, self.G[name + ".weight"],
                                         self.G[name + ".bias"], self.scr.data_ptr(), self.SCRATCH, self.s)

    def _bn_mod(self, name):
        mod = self.mods[name]
        return mod, self.bn_momentum(mod)

    def bn_relu(self, name, y, M, C, z):
        """z (ptr, ld C) = relu(BatchNorm(y [M, C])): batch statistics and running-statistics update in training"""
        mod, mom = self._bn_mod(name)
        st = self.new(2, C)
        self.L.vc_bn_forward_ex(1 if self.train else 0, M, C, y, C, mod.eps, mom, st[0].data_ptr(), st[1].data_ptr(),
                                mod.running_mean.data_ptr(), mod.running_var.data_ptr(), self.P[name + ".weight"],
                                self.P[name + ".bias"], 1, z, C, self.scr.data_ptr(), self.SCRATCH, self.cnt, N_COUNTERS,
                                self.s)
        return st

    def bn_relu_bwd(self, name, dz, y, st, M, C, dy, beta_w=0.0):
        """dy (ptr) = the gradient through ReLU and BatchNorm; the affine's gradients overwritten or added to"""
        self.L.vc_bn_bwd_relu_ex(1 if self.train else 0, M, C, dz, C, y, C, st[0].data_ptr(), st[1].data_ptr(),
                                 self.P[name + ".weight"], self.P[name + ".bias"], dy, C, 0.0, self.G[name + ".weight"],
                                 self.G[name + ".bias"], beta_w, self.scr.data_ptr(), self.SCRATCH, self.cnt, N_COUNTERS,
                                 self.s)

    def bn_pool(self, name, y, nb, H, C, out):
        """out (ptr, [nb, OH, OH, C]) = pool(relu(BatchNorm(y [nb, H, H, C]))): statistics, then one fused pass"""
        mod, mom = self._bn_mod(name)
        st = self.new(2, C)
        self.L.vc_bn_stats_ex(1 if self.train else 0, nb * H * H, C, y, C, mod.eps, mom, st[0].data_ptr(),
                              st[1].data_ptr(), mod.running_mean.data_ptr(), mod.running_var.data_ptr(),
                              self.scr.data_ptr(), self.SCRATCH, self.cnt, N_COUNTERS, self.s)
        OH = H // 2 + 1
        arg = torch.empty(nb * OH * OH * C, dtype=torch.uint8, device=self.dev)
        self.L.vc_maxpool2p_fwd(nb, H, H, C, y, C, st[0].data_ptr(), st[1].data_ptr(), self.P[name + ".weight"],
                                self.P[name + ".bias"], out, arg.data_ptr(), self.s)
        return st, arg

    def bn_pool_bwd(self, name, dout, out, arg, y, st, nb, H, C, dy, beta_w=0.0):
        """dy (ptr) = the gradient of pool(relu(BatchNorm(y))) for dout: pool + ReLU mask, then the BatchNorm"""
        du = self.new(nb * H * H, C)
        self.L.vc_maxpool2p_bwd(nb, H, H, C, dout, arg.data_ptr(), out, du.data_ptr(), C, self.s)
        self.L.vc_bn_bwd_ex(1 if self.train else 0, nb * H * H, C, du.data_ptr(), C, y, C, None, C, st[0].data_ptr(),
                            st[1].data_ptr(), self.P[name + ".weight"], dy, C, 0.0, self.G[name + ".weight"],
                            self.G[name + ".bias"], beta_w, self.scr.data_ptr(), self.SCRATCH, self.cnt, N_COUNTERS,
                            self.s)

    # ------------------------------------------------------------ stages
    def input_rows(self, parts):
        """the NCHW inputs `parts` as channels-last rows [B P P, ld] (their channels side by side), ld = the channel
        count rounded up to 4 floats with the padding written 0 (vc_conv3x3_tap_fwd reads it)"""
        L, B, HW, s = self.L, self.B, self.Pp * self.Pp, self.s
        C = sum(p.shape[1] for p in parts)
        ld = (C + 3) // 4 * 4
        rows = self.new(B * HW, ld)
        c0 = parts[0].shape[1]
        L.vc_nchw_to_nhwc_pad(B, c0, HW, parts[0].data_ptr(), rows.data_ptr(), ld, s)   # columns c0 .. ld - 1: 0
        for p in parts[1:]:
            c = p.shape[1]
            t = self.new(B * HW, c)
            L.vc_nchw_to_nhwc(B, c, HW, p.data_ptr(), t.data_ptr(), s)
            L.vc_add2_2d(B * HW, c, t.data_ptr(), c, None, 0, rows.data_ptr() + F32 * c0, ld, 0.0, s)
            c0 += c
        return rows, C, ld

    def stage_a(self, sfx, parts, out):
        """conv1 .. bn3 + ReLU of one branch; the [B H2 H2, 64] result goes to `out` (ptr)"""
        B, Pp, H2 = self.B, self.Pp, self.H2
        f = FILTERS
        M, M2 = B * Pp * Pp, B * H2 * H2
        rows, C, ld = self.input_rows(parts)
        y1, _ = self.conv3x3("conv1" + sfx, rows.data_ptr(), ld, Pp, C, f[0])
        z1 = self.new(M, f[0])
        st1 = self.bn_relu("bn1" + sfx, y1.data_ptr(), M, f[0], z1.data_ptr())
        y2 = self.conv1x1("conv2" + sfx, z1.data_ptr(), M, f[0], f[1])
        p2 = self.new(M2, f[1])
        st2, arg2 = self.bn_pool("bn2" + sfx, y2.data_ptr(), B, Pp, f[1], p2.data_ptr())
        y3, wt3 = self.conv3x3("conv3" + sfx, p2.data_ptr(), f[1], H2, f[1], f[2])
        st3 = self.bn_relu("bn3" + sfx, y3.data_ptr(), M2, f[2], out)
        return dict(sfx=sfx, rows=rows, C=C, ld=ld, y1=y1, z1=z1, st1=st1, y2=y2, p2=p2, st2=st2, arg2=arg2, y3=y3,
                    wt3=wt3, st3=st3)

    def stage_a_bwd(self, a, dz3):
        """from dz3 (ptr, [B H2 H2, 64]) to the branch's parameter gradients (the inputs are data: no dx)"""
        B, Pp, H2 = self.B, self.Pp, self.H2
        f = FILTERS
        M, M2 = B * Pp * Pp, B * H2 * H2
        sfx = a["sfx"]
        dy3 = self.new(M2, f[2])
        self.bn_relu_bwd("bn3" + sfx, dz3, a["y3"].data_ptr(), a["st3"], M2, f[2], dy3.data_ptr())
        self.conv3x3_wgrad("conv3" + sfx, a["p2"].data_ptr(), f[1], dy3.data_ptr(), H2, f[1], f[2])
        dp2 = self.new(M2, f[1])
        self.L.vc_conv3x3_tap_dgrad(B, H2, H2, f[1], f[2], 1, dy3.data_ptr(), f[2], a["wt3"].data_ptr(), 0.0,
                                    dp2.data_ptr(), f[1], self.scr.data_ptr(), self.SCRATCH, self.s)
        dy2 = self.new(M, f[1])
        self.bn_pool_bwd("bn2" + sfx, dp2.data_ptr(), a["p2"].data_ptr(), a["arg2"], a["y2"].data_ptr(), a["st2"], B, Pp,
                         f[1], dy2.data_ptr())
        dz1 = self.new(M, f[0])
        self.conv1x1_bwd("conv2" + sfx, a["z1"].data_ptr(), dy2.data_ptr(), M, f[0], f[1], dx=dz1.data_ptr())
        dy1 = self.new(M, f[0])
        self.bn_relu_bwd("bn1" + sfx, dz1.data_ptr(), a["y1"].data_ptr(), a["st1"], M, f[0], dy1.data_ptr())
        self.conv3x3_wgrad("conv1" + sfx, a["rows"].data_ptr(), a["ld"], dy1.data_ptr(), Pp, a["C"], f[0])

    def stage_b(self, sfx, x3, out):
        """conv4 - bn4 - ReLU - pool of one branch: x3 (ptr, [B H2 H2, 64]) -> out (ptr, [B H3 H3, 128])"""
        f = FILTERS
        y4 = self.conv1x1("conv4" + sfx, x3, self.B * self.H2 * self.H2, f[2], f[3])
        st4, arg4 = self.bn_pool("bn4" + sfx, y4.data_ptr(), self.B, self.H2, f[3], out)
        return dict(sfx=sfx, x3=x3, y4=y4, st4=st4, arg4=arg4, out=out)

    def stage_b_bwd(self, b, dout, dx3):
        f = FILTERS
        M2 = self.B * self.H2 * self.H2
        sfx = b["sfx"]
        dy4 = self.new(M2, f[3])
        self.bn_pool_bwd("bn4" + sfx, dout, b["out"], b["arg4"], b["y4"].data_ptr(), b["st4"], self.B, self.H2, f[3],
                         dy4.data_ptr())
        self.conv1x1_bwd("conv4" + sfx, b["x3"], dy4.data_ptr(), M2, f[2], f[3], dx=dx3)

    def stage_c(self, sfx, x, K, nseg):
        """conv5 - bn5 - ReLU - conv6 - bn6 - ReLU over `nseg` stacked applications of Ms = B H3 H3 rows each (one GEMM
        per conv; BatchNorm per application, in order); x (tensor [nseg Ms, K]) -> z6 [nseg Ms, 64]"""
        f = FILTERS
        Ms = self.B * self.H3 * self.H3
        R = nseg * Ms
        y5 = self.conv1x1("conv5" + sfx, x.data_ptr(), R, K, f[3])
        z5 = self.new(R, f[3])
        st5 = [self.bn_relu("bn5" + sfx, y5.data_ptr() + F32 * g * Ms * f[3], Ms, f[3], z5.data_ptr() + F32 * g * Ms * f[3])
               for g in range(nseg)]
        y6 = self.conv1x1("conv6" + sfx, z5.data_ptr(), R, f[3], f[2])
        z6 = self.new(R, f[2])
        st6 = [self.bn_relu("bn6" + sfx, y6.data_ptr() + F32 * g * Ms * f[2], Ms, f[2], z6.data_ptr() + F32 * g * Ms * f[2])
               for g in range(nseg)]
        return dict(sfx=sfx, x=x, K=K, nseg=nseg, y5=y5, z5=z5, st5=st5, y6=y6, z6=z6, st6=st6)

    def stage_c_bwd(self, c, dz6):
        """dz6 (tensor [nseg Ms, 64]) -> dx (tensor [nseg Ms, K]); the shared parameters' gradients summed over the
        applications (BatchNorm: application 0 overwrites, the later ones add; the convs: one GEMM over all rows)"""
        f = FILTERS
        Ms = self.B * self.H3 * self.H3
        sfx, nseg, K = c["sfx"], c["nseg"], c["K"]
        R = nseg * Ms
        dy6 = self.new(R, f[2])
        for g in range(nseg):
            o = F32 * g * Ms * f[2]
            self.bn_relu_bwd("bn6" + sfx, dz6.data_ptr() + o, c["y6"].data_ptr() + o, c["st6"][g], Ms, f[2],
                             dy6.data_ptr() + o, beta_w=0.0 if g == 0 else 1.0)
        dz5 = self.new(R, f[3])
        self.conv1x1_bwd("conv6" + sfx, c["z5"].data_ptr(), dy6.data_ptr(), R, f[3], f[2], dx=dz5.data_ptr())
        dy5 = self.new(R, f[3])
        for g in range(nseg):
            o = F32 * g * Ms * f[3]
            self.bn_relu_bwd("bn5" + sfx, dz5.data_ptr() + o, c["y5"].data_ptr() + o, c["st5"][g], Ms, f[3],
                             dy5.data_ptr() + o, beta_w=0.0 if g == 0 else 1.0)
        dx = self.new(R, K)
        self.conv1x1_bwd("conv5" + sfx, c["x"].data_ptr(), dy5.data_ptr(), R, K, f[3], dx=dx.data_ptr())
        return dx

    def head(self, maps, mode):
        """AdaptiveAvgPool2d(1) + conv7 of the G maps (ptrs, [B, H3 H3, 64]) -> logits [G or 1, B, ncls]"""
        m, G = self.m, len(maps)
        HW = self.H3 * self.H3
        C = FILTERS[2]
        n_out = G if mode else 1
        pooled = self.new(n_out * self.B * (C if mode else G * C))
        logits = self.new(n_out, self.B, m.ncls)
        f = list(maps) + [None] * (3 - G)
        self.L.vc_avgpool_head_fwd(self.B, HW, C, G, m.ncls, mode, f[0], f[1], f[2], self.P["conv7.weight"],
                                   self.P["conv7.bias"], pooled.data_ptr(), logits.data_ptr(), self.s)
        self.hd = dict(G=G, mode=mode, pooled=pooled)
        return logits

    def head_bwd(self, dlogits, dmaps):
        m, hd = self.m, self.hd
        d = list(dmaps) + [None] * (3 - hd["G"])
        self.L.vc_avgpool_head_bwd(self.B, self.H3 * self.H3, FILTERS[2], hd["G"], m.ncls, hd["mode"],
                                   dlogits.data_ptr(), self.P["conv7.weight"], hd["pooled"].data_ptr(), d[0], d[1], d[2],
                                   self.G["conv7.weight"], self.G["conv7.bias"], self.s)

    # ------------------------------------------------------------ forward
    def _forward(self):
        return tuple(getattr(self, "_fwd_" + self.m.KIND)().unbind(0))    # [G, B, ncls] -> G outputs

    def count_batches(self):
        # num_batches_tracked += the number of applications, one multi-tensor launch per distinct count (a
        # BatchNorm Cross_fusion_CNN applies two or three times appears once in each list)
        count = {}
        for t in self.nbt:
            count[id(t)] = (t, count.get(id(t), (t, 0))[1] + 1)
        for n in sorted({c for _, c in count.values()}):
            torch._foreach_add_([t for t, c in count.values() if c == n], n)

    def _fwd_early(self):
        f = FILTERS
        M2, M3 = self.B * self.H2 * self.H2, self.B * self.H3 * self.H3
        x3 = self.new(M2, f[2])
        self.a = [self.stage_a("", [self.x1, self.x2], x3.data_ptr())]
        self.x3 = x3
        p4 = self.new(M3, f[3])
        self.b = [self.stage_b("", x3.data_ptr(), p4.data_ptr())]
        self.c = [self.stage_c("", p4, f[3], 1)]
        return self.head([self.c[0]["z6"].data_ptr()], 0)

    def _two_branches(self):
        f = FILTERS
        M2 = self.B * self.H2 * self.H2
        x3 = self.x3 = self.new(2 * M2, f[2])          # the two branches' bn3 outputs, stacked
        self.a = [self.stage_a("_a", [self.x1], x3.data_ptr()),
                  self.stage_a("_b", [self.x2], x3.data_ptr() + F32 * M2 * f[2])]

    def _fwd_middle(self):
        f = FILTERS
        M2, M3 = self.B * self.H2 * self.H2, self.B * self.H3 * self.H3
        self._two_branches()
        x3 = self.x3.data_ptr()
        p4a, p4b = self.new(M3, f[3]), self.new(M3, f[3])
        self.b = [self.stage_b("_a", x3, p4a.data_ptr()), self.stage_b("_b", x3 + F32 * M2 * f[2], p4b.data_ptr())]
        self.p4 = (p4a, p4b)
        xc = self.new(M3, 2 * f[3])
        self.L.vc_cat2_fwd(M3, f[3], f[3], p4a.data_ptr(), f[3], p4b.data_ptr(), f[3], 0, xc.data_ptr(), self.s)
        self.c = [self.stage_c("", xc, 2 * f[3], 1)]
        return self.head([self.c[0]["z6"].data_ptr()], 0)

    def _fwd_late(self):
        f = FILTERS
        M2, M3 = self.B * self.H2 * self.H2, self.B * self.H3 * self.H3
        self._two_branches()
        x3 = self.x3.data_ptr()
        p4a, p4b = self.new(M3, f[3]), self.new(M3, f[3])
        self.b = [self.stage_b("_a", x3, p4a.data_ptr()), self.stage_b("_b", x3 + F32 * M2 * f[2], p4b.data_ptr())]
        self.p4 = (p4a, p4b)
        self.c = [self.stage_c("_a", p4a, f[3], 1), self.stage_c("_b", p4b, f[3], 1)]
        return self.head([c["z6"].data_ptr() for c in self.c], 0)

    def _fwd_cross(self):
        """:278-323.  conv4_a and conv4_b each run once over the stacked [x1; x2] rows; their BatchNorms are applied per
        half in the reference's order bn4_a(x1), bn4_b(x2), bn4_b(x1), bn4_a(x2); conv5 / conv6 run once over the three
        stacked joint layers, bn5 / bn6 per layer in order"""
        L, s = self.L, self.s
        f = FILTERS
        B, H2 = self.B, self.H2
        M2, M3 = B * H2 * H2, B * self.H3 * self.H3
        self._two_branches()
        x3 = self.x3.data_ptr()
        y4a = self.conv1x1("conv4_a", x3, 2 * M2, f[2], f[3])    # rows: conv4_a(x1), conv4_a(x2)
        y4b = self.conv1x1("conv4_b", x3, 2 * M2, f[2], f[3])    # rows: conv4_b(x1), conv4_b(x2)
        half = F32 * M2 * f[3]
        x11, x22, x12, x21 = (self.new(M3, f[3]) for _ in range(4))
        pools = []
        for name, y, seg, out in (("bn4_a", y4a, 0, x11), ("bn4_b", y4b, 1, x22), ("bn4_b", y4b, 0, x12),
                                  ("bn4_a", y4a, 1, x21)):
            st, arg = self.bn_pool(name, y.data_ptr() + seg * half, B, H2, f[3], out.data_ptr())
            pools.append((name, y, seg, out, st, arg))
        self.x4 = dict(y4a=y4a, y4b=y4b, pools=pools)
        # the joint layers, stacked: [x11 + x21 | x22 + x12], [x11 | x12], [x22 | x21]
        K = 2 * f[3]
        xc = self.new(3 * M3, K)
        j = xc.data_ptr()
        L.vc_add2_2d(M3, f[3], x11.data_ptr(), f[3], x21.data_ptr(), f[3], j, K, 0.0, s)
        L.vc_add2_2d(M3, f[3], x22.data_ptr(), f[3], x12.data_ptr(), f[3], j + F32 * f[3], K, 0.0, s)
        L.vc_cat2_fwd(M3, f[3], f[3], x11.data_ptr(), f[3], x12.data_ptr(), f[3], 0, j + F32 * M3 * K, s)
        L.vc_cat2_fwd(M3, f[3], f[3], x22.data_ptr(), f[3], x21.data_ptr(), f[3], 0, j + F32 * 2 * M3 * K, s)
        self.c = [self.stage_c("", xc, K, 3)]
        z6 = self.c[0]["z6"].data_ptr()
        seg = F32 * M3 * f[2]
        return self.head([z6, z6 + seg, z6 + 2 * seg], 1)

    # ------------------------------------------------------------ backward
    def backward(self, dlogits):
        """the flat gradient of every parameter; each is written once (overwritten), the alignment gaps stay zero"""
        grad = self.new_grad()
        getattr(self, "_bwd_" + self.m.KIND)(dlogits)
        self.a = self.b = self.c = self.x4 = self.hd = self.x3 = self.p4 = None
        return grad

    def _bwd_early(self, dlogits):
        f = FILTERS
        M2, M3 = self.B * self.H2 * self.H2, self.B * self.H3 * self.H3
        dz6 = self.new(M3, f[2])
        self.head_bwd(dlogits, [dz6.data_ptr()])
        dp4 = self.stage_c_bwd(self.c[0], dz6)
        dx3 = self.new(M2, f[2])
        self.stage_b_bwd(self.b[0], dp4.data_ptr(), dx3.data_ptr())
        self.stage_a_bwd(self.a[0], dx3.data_ptr())

    def _branches_bwd(self, dp4a, dp4b):
        f = FILTERS
        M2 = self.B * self.H2 * self.H2
        dx3 = self.new(2 * M2, f[2])
        off = F32 * M2 * f[2]
        self.stage_b_bwd(self.b[0], dp4a, dx3.data_ptr())
        self.stage_b_bwd(self.b[1], dp4b, dx3.data_ptr() + off)
        self.stage_a_bwd(self.a[0], dx3.data_ptr())
        self.stage_a_bwd(self.a[1], dx3.data_ptr() + off)

    def _bwd_middle(self, dlogits):
        f = FILTERS
        M3 = self.B * self.H3 * self.H3
        dz6 = self.new(M3, f[2])
        self.head_bwd(dlogits, [dz6.data_ptr()])
        dxc = self.stage_c_bwd(self.c[0], dz6)
        dp4a, dp4b = self.new(M3, f[3]), self.new(M3, f[3])
        self.L.vc_cat2_bwd(M3, f[3], f[3], dxc.data_ptr(), 0, dp4a.data_ptr(), f[3], 0.0, dp4b.data_ptr(), f[3], 0.0,
                           self.s)
        self._branches_bwd(dp4a.data_ptr(), dp4b.data_ptr())

    def _bwd_late(self, dlogits):
        f = FILTERS
        M3 = self.B * self.H3 * self.H3
        dz6a, dz6b = self.new(M3, f[2]), self.new(M3, f[2])
        self.head_bwd(dlogits, [dz6a.data_ptr(), dz6b.data_ptr()])
        dp4a = self.stage_c_bwd(self.c[0], dz6a)
        dp4b = self.stage_c_bwd(self.c[1], dz6b)
        self._branches_bwd(dp4a.data_ptr(), dp4b.data_ptr())

    def _bwd_cross(self, dlogits):
        L, s = self.L, self.s
        f = FILTERS
        B, H2 = self.B, self.H2
        M2, M3 = B * H2 * H2, B * self.H3 * self.H3
        K = 2 * f[3]
        dz6 = self.new(3 * M3, f[2])
        seg = F32 * M3 * f[2]
        self.head_bwd(dlogits, [dz6.data_ptr(), dz6.data_ptr() + seg, dz6.data_ptr() + 2 * seg])
        dxc = self.stage_c_bwd(self.c[0], dz6)
        # joint layers [x11 + x21 | x22 + x12], [x11 | x12], [x22 | x21]: each pooled map feeds two of them
        j0 = dxc.data_ptr()
        j1, j2 = j0 + F32 * M3 * K, j0 + F32 * 2 * M3 * K
        right = F32 * f[3]
        d = {k: self.new(M3, f[3]) for k in ("x11", "x22", "x12", "x21")}
        for k, pa, pb in (("x11", j0, j1), ("x21", j0, j2 + right), ("x22", j0 + right, j2), ("x12", j0 + right, j1 + right)):
            L.vc_add2_2d(M3, f[3], pa, K, pb, K, d[k].data_ptr(), f[3], 0.0, s)
        # the pools and bn4_a / bn4_b per half, in the forward's order (the first application of a BatchNorm overwrites
        # its affine's gradient, the second adds), into the stacked conv4 output gradients
        half = F32 * M2 * f[3]
        dy4 = {"bn4_a": self.new(2 * M2, f[3]), "bn4_b": self.new(2 * M2, f[3])}
        seen = set()
        for (name, y, sg, out, st, arg), k in zip(self.x4["pools"], ("x11", "x22", "x12", "x21")):
            self.bn_pool_bwd(name, d[k].data_ptr(), out.data_ptr(), arg, y.data_ptr() + sg * half, st, B, H2, f[3],
                             dy4[name].data_ptr() + sg * half, beta_w=1.0 if name in seen else 0.0)
            seen.add(name)
        dx3 = self.new(2 * M2, f[2])
        x3 = self.x3.data_ptr()
        self.conv1x1_bwd("conv4_a", x3, dy4["bn4_a"].data_ptr(), 2 * M2, f[2], f[3], dx=dx3.data_ptr())
        self.conv1x1_bwd("conv4_b", x3, dy4["bn4_b"].data_ptr(), 2 * M2, f[2], f[3], dx=dx3.data_ptr(), beta=1.0)
        self.stage_a_bwd(self.a[0], dx3.data_ptr())
        self.stage_a_bwd(self.a[1], dx3.data_ptr() + F32 * M2 * f[2])
