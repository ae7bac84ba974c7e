"""MFT comparison model (the multimodal fusion transformer, HSI + LiDAR) on the MI355X path.

Reference: `model/compare_method/MFT.py` (`MFT` :131-214, `TransformerEncoder` :111-128, `Block` :87-108,
`Mlp` :62-84, `MCrossAttention` :28-59, `HetConv` :15-25), built by `model_utils.py:364-376` (patch 11, FM 16,
Adam lr 5e-4 with weight_decay 5e-3).  The module keeps the reference's parameter tree, creation order and
initialisers, so `state_dict()` has the reference's 58 keys, `.pth` files interchange and the same
`torch.manual_seed` draws the same initial values.

Forward and backward are one hand-written program of HIP kernels (`csrc/mft.hip` + the tap-major 3x3 conv, the
BatchNorm, LayerNorm, GELU, dropout and GEMM entry points) over channels-last rows; the parameters live in one
flat fp32 buffer whose `.grad` the backward fills:

* conv5 (Conv3d 9x3x3, 1 -> 8) writes rows [B*P*P, 8 D] (D = NC - 8) with channel d*8 + c: viewed as
  [B*P*P*D, 8] they are BatchNorm3d(8)'s rows, and conv6 reads them as they are;
* conv6 (HetConv: grouped 3x3 + pointwise) is ONE dense 3x3 conv: `vc_mft_hetconv_pack` writes gwc's blocks on
  the group diagonal and pwc at the centre tap of a tap-major weight in the d*8 + c channel order,
  `vc_conv3x3_tap_*` run it, `vc_mft_hetconv_unpack` takes the two weight gradients out of the dense one;
* the tokenisers, the single-query cross attention and the broadcast residual are `vc_mft_*` kernels.

Dropout (p = 0.1, hard-coded in the reference; five sites: the embeddings :210, proj_drop :58, the Mlp's
dropout twice :81, :83) is applied in training by `vc_dropout_fwd`, seeded and rank-mixed by `program.py`;
each site's p is read from the module tree at forward time.  `HSIOnly` is stored and unused, as in the reference.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import program
from ._lib import lib
from .flat import F32, FlatParams
from .model import N_COUNTERS

LN_EPS = 1e-6        # LayerNorm(dim, eps=1e-6) (MFT.py:91-92, :117)
DIM = 64             # FM * 4 with FM = 16: the tokenisers' 64 is hard-coded in the reference (:164-176)
HEADS = 8
TOKENS = 5           # 1 LiDAR token + 4 HSI tokens
MLP = 512
P_MIN, P_MAX = 5, 28  # vc_mft_conv3d_*: the LDS tile plan (csrc/mft.hip c3_dt)


# ---------------------------------------------------------------- parameter tree (reference names)
class HetConv(nn.Module):
    def __init__(self, in_channels, out_channels, p=64, g=64):
        super().__init__()
        self.gwc = nn.Conv2d(in_channels, out_channels, kernel_size=3, groups=g, padding=1, stride=1)
        self.pwc = nn.Conv2d(in_channels, out_channels, kernel_size=1, groups=p, stride=1)


class MCrossAttention(nn.Module):
    def __init__(self, dim, num_heads=HEADS, proj_drop=0.1):
        super().__init__()
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = head_dim ** -0.5
        self.wq = nn.Linear(head_dim, dim, bias=False)
        self.wk = nn.Linear(head_dim, dim, bias=False)
        self.wv = nn.Linear(head_dim, dim, bias=False)
        self.proj = nn.Linear(dim * num_heads, dim)
        self.proj_drop = nn.Dropout(proj_drop)


class Mlp(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.fc1 = nn.Linear(dim, MLP)
        self.fc2 = nn.Linear(MLP, dim)
        self.act_fn = nn.GELU()
        self.dropout = nn.Dropout(0.1)
        nn.init.xavier_uniform_(self.fc1.weight)
        nn.init.xavier_uniform_(self.fc2.weight)
        nn.init.normal_(self.fc1.bias, std=1e-6)
        nn.init.normal_(self.fc2.bias, std=1e-6)


class Block(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.hidden_size = dim
        self.attention_norm = nn.LayerNorm(dim, eps=LN_EPS)
        self.ffn_norm = nn.LayerNorm(dim, eps=LN_EPS)
        self.ffn = Mlp(dim)
        self.attn = MCrossAttention(dim=dim)


class TransformerEncoder(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.layer = nn.ModuleList()
        self.encoder_norm = nn.LayerNorm(dim, eps=LN_EPS)
        for _ in range(2):
            self.layer.append(Block(dim))   # the reference deep-copies a fresh Block: the same draws


class MFT(FlatParams, nn.Module):
    """Same constructor as the reference `MFT` (MFT.py:131-176); forward(x1 [B,NC,P,P], x2 [B,NCLidar,P,P]) ->
    logits [B, Classes]."""

    def __init__(self, patch_size, FM, NC, NCLidar, Classes, HSIOnly):
        super().__init__()
        _check_supported(patch_size, FM, NC, NCLidar, Classes)
        self.patchsize = patch_size
        self.HSIOnly = HSIOnly
        # creation order = the reference's, so the default initialisation draws the same numbers
        self.conv5 = nn.Sequential(nn.Conv3d(1, 8, (9, 3, 3), padding=(0, 1, 1), stride=1), nn.BatchNorm3d(8),
                                   nn.ReLU())
        self.groups = (FM * 4) // 4 if (8 * (NC - 8)) % FM == 0 else (FM * 4) // 8
        self.conv6 = nn.Sequential(HetConv(8 * (NC - 8), FM * 4, p=1, g=self.groups), nn.BatchNorm2d(FM * 4),
                                   nn.ReLU())
        self.last_BandSize = NC // 2 // 2 // 2
        self.lidarConv = nn.Sequential(nn.Conv2d(NCLidar, 64, 3, 1, 1), nn.BatchNorm2d(64), nn.GELU())
        self.ca = TransformerEncoder(FM * 4)
        self.out3 = nn.Linear(FM * 4, Classes)
        self.position_embeddings = nn.Parameter(torch.randn(1, 4 + 1, FM * 4))
        self.dropout = nn.Dropout(0.1)
        nn.init.xavier_uniform_(self.out3.weight)
        nn.init.normal_(self.out3.bias, std=1e-6)
        self.token_wA = nn.Parameter(torch.empty(1, 4, 64), requires_grad=True)
        nn.init.xavier_normal_(self.token_wA)
        self.token_wV = nn.Parameter(torch.empty(1, 64, 64), requires_grad=True)
        nn.init.xavier_normal_(self.token_wV)
        self.token_wA_L = nn.Parameter(torch.empty(1, 1, 64), requires_grad=True)
        nn.init.xavier_normal_(self.token_wA_L)
        self.token_wV_L = nn.Parameter(torch.empty(1, 64, 64), requires_grad=True)
        nn.init.xavier_normal_(self.token_wV_L)
        self.NC, self.NCLidar, self.ncls = NC, NCLidar, Classes
        self._build_flat()

    def forward(self, x1: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
        if x1.device.type != "cuda" or x2.device.type != "cuda":
            raise RuntimeError("MFT MI355X path: inputs must be on a ROCm (cuda) device; no CPU fallback")
        P = self.patchsize
        if x1.dim() < 2 or x1[0].numel() != self.NC * P * P:
            raise RuntimeError(f"expected x1 [B, {self.NC}, {P}, {P}], got {list(x1.shape)}")
        if x2.dim() < 2 or x2.shape[0] != x1.shape[0] or x2[0].numel() != self.NCLidar * P * P:
            raise RuntimeError(f"expected x2 [B, {self.NCLidar}, {P}, {P}] matching x1, got {list(x2.shape)}")
        B = x1.shape[0]
        x1 = x1.detach().to(torch.float32).reshape(B, self.NC, P, P).contiguous()      # the reshapes of :179-181
        x2 = x2.detach().to(torch.float32).reshape(B, self.NCLidar, P, P).contiguous()
        return program.run(self, _Program, x1, x2)


def _check_supported(patch_size, FM, NC, NCLidar, Classes):
    """reject what a kernel cannot take, at construction"""
    if NC < 9:
        raise ValueError(f"MFT: conv5's 9-band kernel needs NC >= 9 bands, got {NC}")
    if NC > 4096:
        raise ValueError(f"MFT MI355X path: at most 4096 bands (vc_mft_conv3d_*), got {NC}")
    if FM != 16:
        raise ValueError(f"MFT MI355X path: FM must be 16 (the tokenisers' width 64 = FM * 4 is fixed), got {FM}")
    if not P_MIN <= patch_size <= P_MAX:
        raise ValueError(f"MFT MI355X path: patch_size must be in {P_MIN}..{P_MAX} (vc_mft_conv3d_*), got {patch_size}")
    if NCLidar < 1 or Classes < 1:
        raise ValueError("MFT: NCLidar and Classes must be positive")


class _Program(program.Program):
    NAME = "MFT"
    D, LN_EPS = DIM, LN_EPS     # what program.Program.ln reads

    def __init__(self, m: MFT, needs_grad, x1, x2):
        super().__init__(lib(), m, needs_grad, x1, x2)
        self.x1, self.x2 = x1, x2
        self.Pp = m.patchsize
        B = self.B
        # fixed-order partial sums (conv5's weight gradient, the tokenisers, the attention core), split-K slabs
        self.scratch(max(1 << 22, self.L.vc_mft_conv3d_ws_floats(B, m.NC, self.Pp),
                         B * (4 * DIM + DIM * DIM), B * 3 * DIM * 8))
        self.seed_dropout(self.train and any(p > 0 for p in self._drop_ps()))

    def _drop_ps(self):
        m = self.m
        return [m.dropout.p] + [p for blk in m.ca.layer for p in (blk.attn.proj_drop.p, blk.ffn.dropout.p)]

    # ------------------------------------------------------------ forward
    def _forward(self):
        m, L, B, Pp, P, s = self.m, self.L, self.B, self.Pp, self.P, self.s
        HW = Pp * Pp
        M = B * HW
        D = m.NC - 8
        C6 = 8 * D
        scr, ns = self.scr.data_ptr(), self.SCRATCH
        sv = self.sv = {}
        # LiDAR branch (:153-157, :186-188): conv3x3 + BatchNorm + GELU over rows padded to 4 floats
        c2 = m.NCLidar
        x2r, ld2 = self.rows(self.x2, c2, HW)
        wl = self.new(DIM * 9 * ld2)
        L.vc_conv3x3_pack(DIM, c2, 0, P["lidarConv.0.weight"], wl.data_ptr(), 0.0, s)
        yl = self.new(M, DIM)
        L.vc_conv3x3_tap_fwd(B, Pp, Pp, c2, DIM, 1, x2r.data_ptr(), ld2, wl.data_ptr(), P["lidarConv.0.bias"],
                             yl.data_ptr(), DIM, scr, ns, s)
        zl, mean_l, inv_l = self.bn("lidarConv.1", m.lidarConv[1], yl, M, DIM, 0)
        xl = self.new(M, DIM)
        L.vc_gelu_fwd(M * DIM, zl.data_ptr(), xl.data_ptr(), s)
        # HSI branch: conv5 (:136-140, :182-183) into rows [M, 8 D] with channel d*8 + c, BatchNorm3d(8) over the
        # rows viewed [M D, 8], ReLU; conv6 (:142-149) as one dense tap-major 3x3 conv, BatchNorm2d, ReLU
        y5 = self.new(M, C6)
        L.vc_mft_conv3d_fwd(B, m.NC, Pp, self.x1.data_ptr(), P["conv5.0.weight"], P["conv5.0.bias"], y5.data_ptr(),
                            C6, s)
        z5, mean5, inv5 = self.bn("conv5.1", m.conv5[1], y5, M * D, 8, 1)
        wt6 = self.new(DIM * 9 * C6 + DIM)   # the dense weight, then the summed bias
        b6 = wt6.data_ptr() + F32 * DIM * 9 * C6
        L.vc_mft_hetconv_pack(DIM, C6, m.groups, P["conv6.0.gwc.weight"], P["conv6.0.pwc.weight"],
                              P["conv6.0.gwc.bias"], P["conv6.0.pwc.bias"], wt6.data_ptr(), b6, s)
        y6 = self.new(M, DIM)
        L.vc_conv3x3_tap_fwd(B, Pp, Pp, C6, DIM, 1, z5.data_ptr(), C6, wt6.data_ptr(), b6, y6.data_ptr(), DIM, scr,
                             ns, s)
        z6, mean6, inv6 = self.bn("conv6.1", m.conv6[1], y6, M, DIM, 1)
        # tokenisers (:187-209): the LiDAR token is row 0, the 4 HSI tokens rows 1..4; + position embeddings
        T = TOKENS
        X = self.new(B, T, DIM)
        AL, UL, AH, UH = self.new(B, 1, HW), self.new(B, 1, DIM), self.new(B, 4, HW), self.new(B, 4, DIM)
        L.vc_mft_tokpool_fwd(B, HW, 1, xl.data_ptr(), DIM, P["token_wA_L"], P["token_wV_L"],
                             P["position_embeddings"], AL.data_ptr(), UL.data_ptr(), X.data_ptr(), DIM, T * DIM, s)
        L.vc_mft_tokpool_fwd(B, HW, 4, z6.data_ptr(), DIM, P["token_wA"], P["token_wV"],
                             P["position_embeddings"] + F32 * DIM, AH.data_ptr(), UH.data_ptr(),
                             X.data_ptr() + F32 * DIM, DIM, T * DIM, s)
        pe = m.dropout.p if self.train else 0.0
        if pe > 0:
            self.drop("emb", X, None, X, B * T * DIM, pe)
        sv.update(x2r=x2r, yl=yl, zl=zl, mean_l=mean_l, inv_l=inv_l, xl=xl, y5=y5, z5=z5, mean5=mean5, inv5=inv5,
                  wt6=wt6, y6=y6, z6=z6, mean6=mean6, inv6=inv6, AL=AL, UL=UL, AH=AH, UH=UH, pe=pe)
        # the two Blocks (:87-108)
        R = B * T
        self.blocks = []
        for li, blk in enumerate(m.ca.layer):
            pre = f"ca.layer.{li}"
            pd = blk.attn.proj_drop.p if self.train else 0.0
            pf = blk.ffn.dropout.p if self.train else 0.0
            Yn, mu, rs = self.ln(pre + ".attention_norm", X.data_ptr(), R, DIM)
            O, att = self.new(B, HEADS * DIM), self.new(B, HEADS, T)
            L.vc_mft_xattn_fwd(B, T, Yn.data_ptr(), P[pre + ".attn.wq.weight"], P[pre + ".attn.wk.weight"],
                               P[pre + ".attn.wv.weight"], blk.attn.scale, O.data_ptr(), att.data_ptr(), s)
            A1 = self.new(B, DIM)
            self.gemm(0, 1, B, DIM, HEADS * DIM, O.data_ptr(), HEADS * DIM, P[pre + ".attn.proj.weight"], HEADS * DIM,
                      A1.data_ptr(), DIM, bias=P[pre + ".attn.proj.bias"])
            if pd > 0:
                self.drop(f"{li}.attn", A1, None, A1, B * DIM, pd)
            X2 = self.new(B, T, DIM)
            L.vc_mft_bcast_add_fwd(B, T, DIM, X.data_ptr(), A1.data_ptr(), X2.data_ptr(), s)   # x [B,1,64] + h
            Y2, mu2, rs2 = self.ln(pre + ".ffn_norm", X2.data_ptr(), R, DIM)
            Hd = self.new(R, MLP)
            self.gemm(0, 1, R, MLP, DIM, Y2.data_ptr(), DIM, P[pre + ".ffn.fc1.weight"], DIM, Hd.data_ptr(), MLP,
                      bias=P[pre + ".ffn.fc1.bias"])
            G = self.new(R, MLP)
            L.vc_gelu_fwd(R * MLP, Hd.data_ptr(), G.data_ptr(), s)
            X3 = self.new(B, T, DIM)
            if pf > 0:
                self.drop(f"{li}.ff1", G, None, G, R * MLP, pf)
                F2 = self.new(R, DIM)
                self.gemm(0, 1, R, DIM, MLP, G.data_ptr(), MLP, P[pre + ".ffn.fc2.weight"], MLP, F2.data_ptr(), DIM,
                          bias=P[pre + ".ffn.fc2.bias"])
                self.drop(f"{li}.ff2", F2, X2, X3, R * DIM, pf)
            else:
                self.gemm(0, 1, R, DIM, MLP, G.data_ptr(), MLP, P[pre + ".ffn.fc2.weight"], MLP, X3.data_ptr(), DIM,
                          bias=P[pre + ".ffn.fc2.bias"], add=X2.data_ptr(), add_ld=DIM)
            self.blocks.append(dict(X=X, Yn=Yn, mu=mu, rs=rs, O=O, att=att, X2=X2, Y2=Y2, mu2=mu2, rs2=rs2, Hd=Hd, G=G,
                                    pd=pd, pf=pf))
            X = X3
        # encoder_norm, row 0 (:126-128), out3
        Yc, muc, rsc = self.ln("ca.encoder_norm", X.data_ptr(), B, T * DIM)
        logits = self.new(B, m.ncls)
        self.gemm(0, 1, B, m.ncls, DIM, Yc.data_ptr(), DIM, P["out3.weight"], DIM, logits.data_ptr(), m.ncls,
                  bias=P["out3.bias"])
        self.head = (X, Yc, muc, rsc)
        return logits

    # ------------------------------------------------------------ backward
    def backward(self, dlogits):
        """the flat gradient of every parameter; each is written once (overwritten), the alignment gaps stay zero"""
        m, L, B, Pp, P, s = self.m, self.L, self.B, self.Pp, self.P, self.s
        HW = Pp * Pp
        M = B * HW
        D = m.NC - 8
        C6 = 8 * D
        T = TOKENS
        R = B * T
        scr, ns = self.scr.data_ptr(), self.SCRATCH
        sv = self.sv
        tr = 1 if self.train else 0
        grad = self.new_grad()
        G = self.G
        # head
        Xout, Yc, muc, rsc = self.head
        self.gemm(1, 0, m.ncls, DIM, B, dlogits.data_ptr(), m.ncls, Yc.data_ptr(), DIM, G["out3.weight"], DIM,
                  bias_grad=G["out3.bias"])
        dYc = self.new(B, DIM)
        self.gemm(0, 0, B, DIM, m.ncls, dlogits.data_ptr(), m.ncls, P["out3.weight"], DIM, dYc.data_ptr(), DIM)
        dX = self.new(B, T, DIM)
        L.vc_fill(R * DIM, dX.data_ptr(), 0.0, s)
        L.vc_layernorm_bwd(B, DIM, dYc.data_ptr(), DIM, Xout.data_ptr(), T * DIM, P["ca.encoder_norm.weight"],
                           muc.data_ptr(), rsc.data_ptr(), dX.data_ptr(), T * DIM, 0.0, G["ca.encoder_norm.weight"],
                           G["ca.encoder_norm.bias"], 0.0, scr, ns, s)
        for li in reversed(range(len(self.blocks))):
            pre = f"ca.layer.{li}"
            st = self.blocks[li]
            pd, pf = st["pd"], st["pf"]
            # Mlp: X3 = X2 + drop(fc2(drop(gelu(fc1(LN(X2))))))
            dF2 = dX
            if pf > 0:
                dF2 = self.new(R, DIM)
                L.vc_dropout_bwd(R * DIM, dX.data_ptr(), self.masks[f"{li}.ff2"].data_ptr(), pf, dF2.data_ptr(), s)
            self.gemm(1, 0, DIM, MLP, R, dF2.data_ptr(), DIM, st["G"].data_ptr(), MLP, G[pre + ".ffn.fc2.weight"], MLP,
                      bias_grad=G[pre + ".ffn.fc2.bias"])
            dG = self.new(R, MLP)
            self.gemm(0, 0, R, MLP, DIM, dF2.data_ptr(), DIM, P[pre + ".ffn.fc2.weight"], MLP, dG.data_ptr(), MLP)
            if pf > 0:
                L.vc_dropout_bwd(R * MLP, dG.data_ptr(), self.masks[f"{li}.ff1"].data_ptr(), pf, dG.data_ptr(), s)
            dH = self.new(R, MLP)
            L.vc_gelu_bwd(R * MLP, dG.data_ptr(), st["Hd"].data_ptr(), dH.data_ptr(), s)
            self.gemm(1, 0, MLP, DIM, R, dH.data_ptr(), MLP, st["Y2"].data_ptr(), DIM, G[pre + ".ffn.fc1.weight"], DIM,
                      bias_grad=G[pre + ".ffn.fc1.bias"])
            dY2 = self.new(R, DIM)
            self.gemm(0, 0, R, DIM, MLP, dH.data_ptr(), MLP, P[pre + ".ffn.fc1.weight"], DIM, dY2.data_ptr(), DIM)
            dX2 = self.new(B, T, DIM)
            L.vc_layernorm_bwd_res(R, DIM, dY2.data_ptr(), DIM, st["X2"].data_ptr(), DIM, P[pre + ".ffn_norm.weight"],
                                   st["mu2"].data_ptr(), st["rs2"].data_ptr(), dX.data_ptr(), DIM, dX2.data_ptr(), DIM,
                                   G[pre + ".ffn_norm.weight"], G[pre + ".ffn_norm.bias"], 0.0, scr, ns, s)
            # attention: X2[b,t] = X[b,t] + drop(proj(core(LN(X))))[b]: the broadcast's backward sums the rows
            dA1 = self.new(B, DIM)
            L.vc_mft_bcast_add_bwd(B, T, DIM, dX2.data_ptr(), dA1.data_ptr(), s)
            if pd > 0:
                L.vc_dropout_bwd(B * DIM, dA1.data_ptr(), self.masks[f"{li}.attn"].data_ptr(), pd, dA1.data_ptr(), s)
            E = HEADS * DIM
            self.gemm(1, 0, DIM, E, B, dA1.data_ptr(), DIM, st["O"].data_ptr(), E, G[pre + ".attn.proj.weight"], E,
                      bias_grad=G[pre + ".attn.proj.bias"])
            dO = self.new(B, E)
            self.gemm(0, 0, B, E, DIM, dA1.data_ptr(), DIM, P[pre + ".attn.proj.weight"], E, dO.data_ptr(), E)
            dYn = self.new(R, DIM)
            L.vc_mft_xattn_bwd(B, T, st["Yn"].data_ptr(), P[pre + ".attn.wq.weight"], P[pre + ".attn.wk.weight"],
                               P[pre + ".attn.wv.weight"], st["att"].data_ptr(), dO.data_ptr(),
                               m.ca.layer[li].attn.scale, dYn.data_ptr(), G[pre + ".attn.wq.weight"],
                               G[pre + ".attn.wk.weight"], G[pre + ".attn.wv.weight"], scr, ns, s)
            dX1 = self.new(B, T, DIM)
            L.vc_layernorm_bwd_res(R, DIM, dYn.data_ptr(), DIM, st["X"].data_ptr(), DIM,
                                   P[pre + ".attention_norm.weight"], st["mu"].data_ptr(), st["rs"].data_ptr(),
                                   dX2.data_ptr(), DIM, dX1.data_ptr(), DIM, G[pre + ".attention_norm.weight"],
                                   G[pre + ".attention_norm.bias"], 0.0, scr, ns, s)
            dX = dX1
        # embeddings: X0 = dropout(cat(lidar token, HSI tokens) + position_embeddings)
        if sv["pe"] > 0:
            L.vc_dropout_bwd(R * DIM, dX.data_ptr(), self.masks["emb"].data_ptr(), sv["pe"], dX.data_ptr(), s)
        L.vc_colsum(B, T * DIM, dX.data_ptr(), T * DIM, G["position_embeddings"], 0.0, scr, ns, s)
        dz6, dxl = self.new(M, DIM), self.new(M, DIM)
        L.vc_mft_tokpool_bwd(B, HW, 4, sv["z6"].data_ptr(), DIM, P["token_wA"], P["token_wV"], sv["AH"].data_ptr(),
                             sv["UH"].data_ptr(), dX.data_ptr() + F32 * DIM, DIM, T * DIM, dz6.data_ptr(), DIM,
                             G["token_wA"], G["token_wV"], scr, ns, s)
        L.vc_mft_tokpool_bwd(B, HW, 1, sv["xl"].data_ptr(), DIM, P["token_wA_L"], P["token_wV_L"], sv["AL"].data_ptr(),
                             sv["UL"].data_ptr(), dX.data_ptr(), DIM, T * DIM, dxl.data_ptr(), DIM, G["token_wA_L"],
                             G["token_wV_L"], scr, ns, s)
        # LiDAR branch: GELU, BatchNorm, conv (x2 is data: no input gradient)
        dzl, dyl = self.new(M, DIM), self.new(M, DIM)
        L.vc_gelu_bwd(M * DIM, dxl.data_ptr(), sv["zl"].data_ptr(), dzl.data_ptr(), s)
        L.vc_bn_bwd_ex(tr, M, DIM, dzl.data_ptr(), DIM, sv["yl"].data_ptr(), DIM, None, DIM, sv["mean_l"].data_ptr(),
                       sv["inv_l"].data_ptr(), P["lidarConv.1.weight"], dyl.data_ptr(), DIM, 0.0,
                       G["lidarConv.1.weight"], G["lidarConv.1.bias"], 0.0, scr, ns, self.cnt, N_COUNTERS, s)
        c2 = m.NCLidar
        L.vc_conv3x3_tap_wgrad_oihw(B, Pp, Pp, c2, DIM, 1, sv["x2r"].data_ptr(), (c2 + 3) // 4 * 4, dyl.data_ptr(), DIM,
                                    G["lidarConv.0.weight"], G["lidarConv.0.bias"], scr, ns, s)
        # HSI branch: BatchNorm2d + ReLU, conv6 (dense weight gradient -> gwc / pwc; both biases take the same
        # column sums), BatchNorm3d + ReLU, conv5 (x1 is data: no input gradient)
        dy6 = self.new(M, DIM)
        L.vc_bn_bwd_relu_ex(tr, M, DIM, dz6.data_ptr(), DIM, sv["y6"].data_ptr(), DIM, sv["mean6"].data_ptr(),
                            sv["inv6"].data_ptr(), P["conv6.1.weight"], P["conv6.1.bias"], dy6.data_ptr(), DIM, 0.0,
                            G["conv6.1.weight"], G["conv6.1.bias"], 0.0, scr, ns, self.cnt, N_COUNTERS, s)
        dwt = self.new(DIM * 9 * C6)
        L.vc_conv3x3_tap_wgrad(B, Pp, Pp, C6, DIM, 1, sv["z5"].data_ptr(), C6, dy6.data_ptr(), DIM, dwt.data_ptr(),
                               scr, ns, s)
        L.vc_mft_hetconv_unpack(DIM, C6, m.groups, dwt.data_ptr(), G["conv6.0.gwc.weight"], G["conv6.0.pwc.weight"],
                                s)
        L.vc_colsum(M, DIM, dy6.data_ptr(), DIM, G["conv6.0.gwc.bias"], 0.0, scr, ns, s)
        L.vc_colsum(M, DIM, dy6.data_ptr(), DIM, G["conv6.0.pwc.bias"], 0.0, scr, ns, s)
        dz5 = self.new(M, C6)
        L.vc_conv3x3_tap_dgrad(B, Pp, Pp, C6, DIM, 1, dy6.data_ptr(), DIM, sv["wt6"].data_ptr(), 0.0, dz5.data_ptr(),
                               C6, scr, ns, s)
        dy5 = self.new(M, C6)
        L.vc_bn_bwd_relu_ex(tr, M * D, 8, dz5.data_ptr(), 8, sv["y5"].data_ptr(), 8, sv["mean5"].data_ptr(),
                            sv["inv5"].data_ptr(), P["conv5.1.weight"], P["conv5.1.bias"], dy5.data_ptr(), 8, 0.0,
                            G["conv5.1.weight"], G["conv5.1.bias"], 0.0, scr, ns, self.cnt, N_COUNTERS, s)
        L.vc_mft_conv3d_wgrad(B, m.NC, Pp, self.x1.data_ptr(), dy5.data_ptr(), C6, G["conv5.0.weight"],
                              G["conv5.0.bias"], scr, ns, s)
        self.sv, self.blocks, self.head = {}, [], None
        return grad
