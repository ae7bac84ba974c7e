"""HCTnet comparison model (the dual-branch cross-token transformer, HSI + LiDAR) on the MI355X path.

Reference: `model/compare_method/HCTnet.py` (`HCTnet` :224-367, `FusionEncoder` :175-203, `CT_Transformer` :152-171,
`CTAttention` :96-131, `Transformer` :205-219, `Attention` :56-94, `MLP_Block` :42-54), built by
`model_utils.py:351-363` (patch 11, 6 tokens, 8 heads, Adam lr 1e-4, applyPCA to 3 components).  The module keeps the
reference's parameter tree, creation order and initialisers, so `state_dict()` has the reference's 77 keys, `.pth` files
interchange and the same `torch.manual_seed` draws the same initial values; `transformer` is stored and unused, as in
the reference (its 12 parameters get a zero gradient).

The reference passes no band count: its Conv3d(1, 8, 3x3x3) is followed by Conv2d(8, 64) on the `(c h)` reshape, which
has 8 channels only at HSI depth 3 -- what applyPCA(., 3) produces.  So the model takes x1 [B, 3, P, P] and
x2 [B, in_channels, P, P]; at depth 3 the 3-D conv is a valid 3x3 conv 3 -> 8 and BatchNorm3d(8) an 8-channel BatchNorm.

Forward and backward are one hand-written program of HIP kernels over channels-last rows: the
three valid convs through `vc_conv3x3_tap_*` + `vc_bn_*_ex`, then `vc_hct_tokpool_*` (both sources share the tokeniser's
parameters: the two backward calls' partials are reduced together), `vc_hct_encoder_*` (both branches' encoder layer,
one launch) and `vc_hct_ctattn_*` (both cross-token directions, one launch), the head's LayerNorm + Linear on the two
cls rows as 2 B rows.  The parameters live in one flat fp32 buffer whose `.grad` the backward fills.

Dropout (12 sites, p = 0.1 in the reference: the two embeddings; per branch the attention output and the MLP twice; per
direction the attention probabilities and to_out) is applied in training inside those kernels with `vc_dropout_fwd`'s
hash, seeded and rank-mixed by `program.py`; each site's p is read from the module tree at forward time and every keep
mask is kept as bytes (`_Program.masks`).

Patch sides 5..30: the tokeniser keeps a sample's L x (P-2)^2 softmax weights twice in LDS in its backward
(2 * 8 * 784 floats = 49 KB of the 64 KB a block may declare statically).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import program
from ._lib import lib
from .flat import F32, FlatParams
from .model import N_COUNTERS

LN_EPS = 1e-5        # nn.LayerNorm's default (HCTnet.py:35, :313)
DIM = 64
HEADS = 8
MLP_DIM = 8
CT_DIM_HEAD = 64
L_MAX = 8            # vc_hct_tokpool_*: one wave per token
P_MIN, P_MAX = 5, 30  # vc_hct_tokpool_*: (P - 2)^2 <= 784 pixels in LDS
ENC_FLOATS = 17992    # VC_HCT_ENC_FLOATS: one Transformer layer's packed parameters
CT_FLOATS = 131264    # VC_HCT_CT_FLOATS: one cross-token direction's packed parameters


# ---------------------------------------------------------------- parameter tree (reference names)
class Residual(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn


class LayerNormalize(nn.Module):
    def __init__(self, dim, fn):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.fn = fn


class MLP_Block(nn.Module):
    def __init__(self, dim, hidden_dim, dropout=0.1):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(dim, hidden_dim), nn.GELU(), nn.Dropout(dropout), nn.Linear(hidden_dim, dim),
                                 nn.Dropout(dropout))


class Attention(nn.Module):
    def __init__(self, dim, heads=8, dropout=0.1):
        super().__init__()
        self.heads = heads
        self.scale = dim ** -0.5   # the model width, not the head width (HCTnet.py:61)
        self.to_qkv = nn.Linear(dim, dim * 3, bias=True)
        self.nn1 = nn.Linear(dim, dim)
        self.do1 = nn.Dropout(dropout)


class CTAttention(nn.Module):
    def __init__(self, dim, heads=8, dim_head=64, dropout=0.1):
        super().__init__()
        inner = dim_head * heads
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.attend = nn.Softmax(dim=-1)
        self.dropout = nn.Dropout(dropout)
        self.to_q = nn.Linear(dim, inner, bias=False)
        self.to_kv = nn.Linear(dim, inner * 2, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, dim), nn.Dropout(dropout))


class ProjectInOut(nn.Module):
    def __init__(self, dim_in, dim_out, fn):
        super().__init__()
        self.fn = fn
        self.project_in = nn.Identity()    # dim_in == dim_out on this path (checked at construction)
        self.project_out = nn.Identity()


class CT_Transformer(nn.Module):
    def __init__(self, h_dim, l_dim, depth, heads, dim_head, dropout):
        super().__init__()
        self.layers = nn.ModuleList([])
        for _ in range(depth):
            self.layers.append(nn.ModuleList([
                ProjectInOut(h_dim, l_dim, LayerNormalize(l_dim, CTAttention(l_dim, heads, dim_head, dropout))),
                ProjectInOut(l_dim, h_dim, LayerNormalize(h_dim, CTAttention(h_dim, heads, dim_head, dropout)))]))


class Transformer(nn.Module):
    def __init__(self, dim, depth, heads, mlp_dim, dropout):
        super().__init__()
        self.layers = nn.ModuleList([])
        for _ in range(depth):
            self.layers.append(nn.ModuleList([
                Residual(LayerNormalize(dim, Attention(dim, heads=heads, dropout=dropout))),
                Residual(LayerNormalize(dim, MLP_Block(dim, mlp_dim, dropout=dropout)))]))


class FusionEncoder(nn.Module):
    def __init__(self, *, depth, h_dim, l_dim, h_enc_params, l_enc_params, ct_attn_heads, ct_attn_depth,
                 ct_attn_dim_head=64, dropout=0.):
        super().__init__()
        self.layers = nn.ModuleList([])
        for _ in range(depth):
            self.layers.append(nn.ModuleList([
                Transformer(dim=h_dim, dropout=dropout, **h_enc_params),
                Transformer(dim=l_dim, dropout=dropout, **l_enc_params),
                CT_Transformer(h_dim, l_dim, ct_attn_depth, ct_attn_heads, ct_attn_dim_head, dropout)]))


class HCTnet(FlatParams, nn.Module):
    """Same constructor as the reference `HCTnet` (HCTnet.py:225-250); forward(x1 [B,3,P,P], x2 [B,in_channels,P,P]) ->
    logits [B, num_classes], 5 <= P <= 30."""

    def __init__(self, in_channels=1, num_classes=6, num_tokens=4, dim=64, heads=8, mlp_dim=8, h_dim=64, l_dim=64,
                 depth=1, dropout=0.1, emb_dropout=0.1, h_enc_depth=1, h_enc_heads=8, h_enc_mlp_dim=8, l_enc_depth=1,
                 l_enc_heads=8, l_enc_mlp_dim=8, ct_attn_depth=1, ct_attn_heads=8, ct_attn_dim_head=64):
        super().__init__()
        _check_supported(in_channels, num_classes, num_tokens, dim, heads, mlp_dim, h_dim, l_dim, depth, dropout,
                         emb_dropout, h_enc_depth, h_enc_heads, h_enc_mlp_dim, l_enc_depth, l_enc_heads, l_enc_mlp_dim,
                         ct_attn_depth, ct_attn_heads, ct_attn_dim_head)
        self.L = num_tokens
        self.cT = dim
        # creation order = the reference's, so the default initialisation draws the same numbers
        self.conv3d_features = nn.Sequential(nn.Conv3d(1, 8, kernel_size=(3, 3, 3)), nn.BatchNorm3d(8), nn.ReLU())
        self.conv2d_features = nn.Sequential(nn.Conv2d(8, 64, kernel_size=(3, 3)), nn.BatchNorm2d(64), nn.ReLU())
        self.conv2d_features2 = nn.Sequential(nn.Conv2d(in_channels, 64, kernel_size=(3, 3)), nn.BatchNorm2d(64),
                                              nn.ReLU())
        self.token_wA = nn.Parameter(torch.empty(1, self.L, dim), requires_grad=True)
        nn.init.xavier_normal_(self.token_wA)
        self.token_wV = nn.Parameter(torch.empty(1, dim, self.cT), requires_grad=True)
        nn.init.xavier_normal_(self.token_wV)
        self.pos_embedding = nn.Parameter(torch.empty(1, num_tokens + 1, dim))
        nn.init.normal_(self.pos_embedding, std=.02)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.dropout = nn.Dropout(emb_dropout)
        self.fusion_encoder = FusionEncoder(
            depth=depth, h_dim=h_dim, l_dim=l_dim, ct_attn_heads=ct_attn_heads, ct_attn_dim_head=ct_attn_dim_head,
            ct_attn_depth=ct_attn_depth, h_enc_params=dict(depth=h_enc_depth, heads=h_enc_heads, mlp_dim=h_enc_mlp_dim),
            l_enc_params=dict(depth=l_enc_depth, heads=l_enc_heads, mlp_dim=l_enc_mlp_dim), dropout=dropout)
        self.transformer = Transformer(dim, depth, heads, mlp_dim, dropout)   # never used by forward (:346-361)
        self.mlp_head = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, num_classes))
        self.in_channels, self.ncls = in_channels, num_classes
        self._build_flat()
        self._packed = _packed_offsets(self)

    def forward(self, x1: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
        if x1.device.type != "cuda" or x2.device.type != "cuda":
            raise RuntimeError("HCTnet MI355X path: inputs must be on a ROCm (cuda) device; no CPU fallback")
        if x1.dim() != 4 or x1.shape[1] != 3 or x1.shape[2] != x1.shape[3]:
            raise RuntimeError(f"expected x1 [B, 3, P, P] (the HSI cube reduced to 3 components), got {list(x1.shape)}")
        P = x1.shape[2]
        if not P_MIN <= P <= P_MAX:
            raise RuntimeError(f"HCTnet MI355X path: the patch side must be in {P_MIN}..{P_MAX}, got {P}")
        if x2.dim() != 4 or tuple(x2.shape) != (x1.shape[0], self.in_channels, P, P):
            raise RuntimeError(f"expected x2 [B, {self.in_channels}, {P}, {P}] matching x1, got {list(x2.shape)}")
        if x1.shape[0] < 1:
            raise RuntimeError("empty batch")
        x1 = x1.detach().to(torch.float32).contiguous()
        x2 = x2.detach().to(torch.float32).contiguous()
        return program.run(self, _Program, x1, x2)


def _check_supported(in_channels, num_classes, num_tokens, dim, heads, mlp_dim, h_dim, l_dim, depth, dropout,
                     emb_dropout, h_enc_depth, h_enc_heads, h_enc_mlp_dim, l_enc_depth, l_enc_heads, l_enc_mlp_dim,
                     ct_attn_depth, ct_attn_heads, ct_attn_dim_head):
    """reject what a kernel cannot take, at construction"""
    pre = "HCTnet MI355X path: "
    if not 1 <= num_tokens <= L_MAX:
        raise ValueError(f"{pre}num_tokens must be in 1..{L_MAX} (vc_hct_tokpool_*), got {num_tokens}")
    if (dim, h_dim, l_dim) != (DIM, DIM, DIM):
        raise ValueError(f"{pre}dim, h_dim and l_dim must be {DIM}, got {(dim, h_dim, l_dim)}")
    if (depth, h_enc_depth, l_enc_depth, ct_attn_depth) != (1, 1, 1, 1):
        raise ValueError(f"{pre}depth, h_enc_depth, l_enc_depth and ct_attn_depth must be 1, got "
                         f"{(depth, h_enc_depth, l_enc_depth, ct_attn_depth)}")
    if (h_enc_heads, l_enc_heads, ct_attn_heads) != (HEADS, HEADS, HEADS):
        raise ValueError(f"{pre}h_enc_heads, l_enc_heads and ct_attn_heads must be {HEADS} (vc_hct_encoder_*, "
                         f"vc_hct_ctattn_*), got {(h_enc_heads, l_enc_heads, ct_attn_heads)}")
    if (h_enc_mlp_dim, l_enc_mlp_dim) != (MLP_DIM, MLP_DIM):
        raise ValueError(f"{pre}h_enc_mlp_dim and l_enc_mlp_dim must be {MLP_DIM} (vc_hct_encoder_*), got "
                         f"{(h_enc_mlp_dim, l_enc_mlp_dim)}")
    if ct_attn_dim_head != CT_DIM_HEAD:
        raise ValueError(f"{pre}ct_attn_dim_head must be {CT_DIM_HEAD} (vc_hct_ctattn_*), got {ct_attn_dim_head}")
    if heads < 1 or mlp_dim < 1:
        raise ValueError("HCTnet: heads and mlp_dim (the unused transformer's) must be positive")
    if in_channels < 1 or num_classes < 1:
        raise ValueError("HCTnet: in_channels and num_classes must be positive")
    if not (0.0 <= dropout < 1.0 and 0.0 <= emb_dropout < 1.0):
        raise ValueError("HCTnet: dropout and emb_dropout must be in [0, 1)")


ENC_NAMES = ("0.fn.norm.weight", "0.fn.norm.bias", "0.fn.fn.to_qkv.weight", "0.fn.fn.to_qkv.bias", "0.fn.fn.nn1.weight",
             "0.fn.fn.nn1.bias", "1.fn.norm.weight", "1.fn.norm.bias", "1.fn.fn.net.0.weight", "1.fn.fn.net.0.bias",
             "1.fn.fn.net.3.weight", "1.fn.fn.net.3.bias")
CT_NAMES = ("fn.norm.weight", "fn.norm.bias", "fn.fn.to_q.weight", "fn.fn.to_kv.weight", "fn.fn.to_out.0.weight",
            "fn.fn.to_out.0.bias")


def _packed_offsets(m):
    """the flat offsets of the four packed parameter blocks the fused kernels read (each must be contiguous in the
    flat buffer, in module order, and start 16-B aligned: every size is a multiple of 4 floats, so it is)"""
    named = dict(nn.Module.named_parameters(m))
    out = {}
    for key, pfx, names, total in (
            ("enc0", "fusion_encoder.layers.0.0.layers.0.", ENC_NAMES, ENC_FLOATS),
            ("enc1", "fusion_encoder.layers.0.1.layers.0.", ENC_NAMES, ENC_FLOATS),
            ("ct0", "fusion_encoder.layers.0.2.layers.0.0.", CT_NAMES, CT_FLOATS),
            ("ct1", "fusion_encoder.layers.0.2.layers.0.1.", CT_NAMES, CT_FLOATS)):
        off = m._poff[pfx + names[0]]
        o = off
        for n in names:
            if m._poff[pfx + n] != o:
                raise RuntimeError(f"HCTnet: {pfx + n} is not packed behind its predecessor in the flat buffer")
            o += named[pfx + n].numel()
        if o - off != total or off % 4:
            raise RuntimeError(f"HCTnet: the packed block {pfx} has {o - off} floats at offset {off}, expected {total}")
        out[key] = off
    return out


class _Program(program.Program):
    NAME = "HCTnet"

    def __init__(self, m: HCTnet, needs_grad, x1, x2):
        super().__init__(lib(), m, needs_grad, x1, x2)
        self.x1, self.x2 = x1, x2
        self.Pp = x1.shape[2]
        # split-K slabs; with a backward to come, its per-sample weight-gradient partials (both cross-token
        # directions are the largest).  Grow-only, and the kernels are told the buffer's own size
        self.scratch(max(1 << 22, 2 * self.B * CT_FLOATS if needs_grad else 0), grow=True)
        base = m._flat_store.data_ptr()
        self.W = {k: base + F32 * o for k, o in m._packed.items()}
        self.seed_dropout(self.train and any(p > 0 for p in self._drop_ps()))

    def _enc_ps(self):
        """(attention output, MLP hidden, MLP output) p of both branches; 0 in eval"""
        out = []
        for b in (0, 1):
            lay = self.m.fusion_encoder.layers[0][b].layers[0]
            ps = (lay[0].fn.fn.do1.p, lay[1].fn.fn.net[2].p, lay[1].fn.fn.net[4].p)
            out += [float(p) if self.train else 0.0 for p in ps]
        return out

    def _ct_ps(self):
        """(probabilities, to_out) p of both directions; 0 in eval"""
        out = []
        for d in (0, 1):
            att = self.m.fusion_encoder.layers[0][2].layers[0][d].fn.fn
            out += [float(p) if self.train else 0.0 for p in (att.dropout.p, att.to_out[1].p)]
        return out

    def _drop_ps(self):
        return [self.m.dropout.p] + self._enc_ps() + self._ct_ps()

    def site_seed(self, k):
        return (self.seed + 1000003 * k) % (1 << 63)

    def conv(self, pfx, x, ldx, H, C, O):
        """valid 3x3 conv of channels-last rows x [B, H, H, C] (ld ldx) -> (y [B (H-2)^2, O], the tap-major weight)"""
        L, B = self.L, self.B
        wt = self.pack3x3(pfx + ".weight", O, C)
        y = self.new(B * (H - 2) * (H - 2), O)
        L.vc_conv3x3_tap_fwd(B, H, H, C, O, 0, x.data_ptr(), ldx, wt.data_ptr(), self.P[pfx + ".bias"], y.data_ptr(), O,
                             self.scr.data_ptr(), self.SCRATCH, self.s)
        return y, wt

    # ------------------------------------------------------------ forward
    def _forward(self):
        m, L, B, Pp, P, s = self.m, self.L, self.B, self.Pp, self.P, self.s
        H1, H2 = Pp - 2, Pp - 4
        M1, M2 = B * H1 * H1, B * H2 * H2
        sv = self.sv = {}
        tr = self.train
        # HSI branch (:317-321): the 3-D conv at depth 3 is a valid 3x3 conv 3 -> 8 (its [8,1,3,3,3] weight read as
        # [8,3,3,3]), BatchNorm3d(8) an 8-channel BatchNorm of the rows; then the valid 3x3 conv 8 -> 64
        x1r, ld1 = self.rows(self.x1, 3, Pp * Pp)
        y3, _ = self.conv("conv3d_features.0", x1r, ld1, Pp, 3, 8)
        z3, mean3, inv3 = self.bn("conv3d_features.1", m.conv3d_features[1], y3, M1, 8)
        y2, wt2 = self.conv("conv2d_features.0", z3, 8, H1, 8, DIM)
        z2, mean2, inv2 = self.bn("conv2d_features.1", m.conv2d_features[1], y2, M2, DIM)
        # LiDAR branch (:323-324)
        c2 = m.in_channels
        x2r, ld2 = self.rows(self.x2, c2, Pp * Pp)
        yl, _ = self.conv("conv2d_features2.0", x2r, ld2, Pp, c2, DIM)
        zl, meanl, invl = self.bn("conv2d_features2.1", m.conv2d_features2[1], yl, M1, DIM)
        # tokens (:326-353): both sources through the one tokeniser into X0 [2][B, T, 64]
        Lt, T = m.L, m.L + 1
        self.T = T
        X0 = self.new(2, B, T, DIM)
        pe = float(m.dropout.p) if tr else 0.0
        AH, UH, AL, UL = self.new(B, Lt, H2 * H2), self.new(B, Lt, DIM), self.new(B, Lt, H1 * H1), self.new(B, Lt, DIM)
        mk_h = self.bytes(B, T, DIM) if tr else None
        mk_l = self.bytes(B, T, DIM) if tr else None
        ds = self.dseed
        for k, (src, HW, A, U, mk) in enumerate(((z2, H2 * H2, AH, UH, mk_h), (zl, H1 * H1, AL, UL, mk_l))):
            seed = (ds.cur_ptr, 1000003 * k) if ds is not None else (self.site_seed(k),)
            (L.vc_hct_tokpool_fwd_ds if ds is not None else L.vc_hct_tokpool_fwd)(
                B, HW, Lt, src.data_ptr(), DIM, P["token_wA"], P["token_wV"], P["cls_token"], P["pos_embedding"], pe,
                *seed, A.data_ptr(), U.data_ptr(), X0[k].data_ptr(), mk.data_ptr() if mk is not None else None, s)
        # the two encoder layers (:200), one launch
        ep = self._enc_ps()
        mk_e = self.bytes(2, B, T * (2 * DIM + MLP_DIM)) if tr else None
        X1 = self.new(2, B, T, DIM)
        st = B * T * DIM
        seed = (ds.cur_ptr, 1000003 * 2) if ds is not None else (self.site_seed(2),)
        (L.vc_hct_encoder_fwd_ds if ds is not None else L.vc_hct_encoder_fwd)(
            B, T, X0.data_ptr(), st, self.W["enc0"], self.W["enc1"], *ep, *seed, X1.data_ptr(), st,
            mk_e.data_ptr() if tr else None, s)
        # the cross-token step (:162-171), both directions in one launch; only the cls rows go on to the head
        cp = self._ct_ps()
        mk_c = self.bytes(2, B, HEADS * T + DIM) if tr else None
        C = self.new(2 * B, DIM)
        seed = (ds.cur_ptr, 1000003 * 3) if ds is not None else (self.site_seed(3),)
        (L.vc_hct_ctattn_fwd_ds if ds is not None else L.vc_hct_ctattn_fwd)(
            B, T, X1.data_ptr(), st, self.W["ct0"], self.W["ct1"], *cp, *seed, C.data_ptr(),
            mk_c.data_ptr() if tr else None, s)
        # mlp_head on both cls rows (2 B rows), summed (:362-364)
        Yc, mu, rs = self.new(2 * B, DIM), self.new(2 * B), self.new(2 * B)
        L.vc_layernorm_fwd(2 * B, DIM, C.data_ptr(), DIM, P["mlp_head.0.weight"], P["mlp_head.0.bias"], LN_EPS,
                           Yc.data_ptr(), DIM, mu.data_ptr(), rs.data_ptr(), s)
        n = m.ncls
        L2 = self.new(2 * B, n)
        self.gemm(0, 1, 2 * B, n, DIM, Yc.data_ptr(), DIM, P["mlp_head.1.weight"], DIM, L2.data_ptr(), n,
                  bias=P["mlp_head.1.bias"])
        logits = self.new(B, n)
        L.vc_add2_2d(B, n, L2.data_ptr(), n, L2.data_ptr() + F32 * B * n, n, logits.data_ptr(), n, 0.0, s)
        if tr:
            self.masks = self._split_masks(mk_h, mk_l, mk_e, mk_c)
        sv.update(x1r=x1r, ld1=ld1, y3=y3, z3=z3, mean3=mean3, inv3=inv3, y2=y2, wt2=wt2, z2=z2, mean2=mean2, inv2=inv2,
                  x2r=x2r, ld2=ld2, yl=yl, zl=zl, meanl=meanl, invl=invl, AH=AH, UH=UH, AL=AL, UL=UL, X0=X0, X1=X1, C=C,
                  Yc=Yc, mu=mu, rs=rs, pe=pe, ep=ep, cp=cp, mk_h=mk_h, mk_l=mk_l, mk_e=mk_e, mk_c=mk_c)
        return logits

    def _split_masks(self, mk_h, mk_l, mk_e, mk_c):
        """views of the kernels' mask bytes under the 12 sites' names (tests/hct_oracle.py's)"""
        B, T = self.B, self.T
        out = {"emb.h": mk_h, "emb.l": mk_l}
        a, h = T * DIM, T * MLP_DIM
        for b, name in enumerate("hl"):
            out[f"enc.{name}.attn"] = mk_e[b, :, :a].reshape(B, T, DIM)
            out[f"enc.{name}.ff1"] = mk_e[b, :, a:a + h].reshape(B, T, MLP_DIM)
            out[f"enc.{name}.ff2"] = mk_e[b, :, a + h:].reshape(B, T, DIM)
            out[f"ct.{name}.prob"] = mk_c[b, :, :HEADS * T].reshape(B, HEADS, 1, T)
            out[f"ct.{name}.out"] = mk_c[b, :, HEADS * T:].reshape(B, 1, DIM)
        return out

    # ------------------------------------------------------------ backward
    def backward(self, dlogits):
        """the flat gradient of every parameter; each is written once (overwritten), the unused transformer's stay 0"""
        m, L, B, Pp, P, s = self.m, self.L, self.B, self.Pp, self.P, self.s
        H1, H2 = Pp - 2, Pp - 4
        M1, M2 = B * H1 * H1, B * H2 * H2
        T, Lt, n = self.T, m.L, m.ncls
        scr, ns = self.scr.data_ptr(), self.SCRATCH
        sv = self.sv
        tr = 1 if self.train else 0
        grad = self.new_grad()
        G = self.G
        GW = {k: grad.data_ptr() + F32 * o for k, o in m._packed.items()}

        def ptr(t):
            return t.data_ptr() if t is not None else None

        # head: both halves of the 2 B rows take the same dlogits
        dl2 = self.new(2 * B, n)
        for half in (0, 1):
            L.vc_add2_2d(B, n, dlogits.data_ptr(), n, None, 0, dl2.data_ptr() + F32 * half * B * n, n, 0.0, s)
        self.gemm(1, 0, n, DIM, 2 * B, dl2.data_ptr(), n, sv["Yc"].data_ptr(), DIM, G["mlp_head.1.weight"], DIM,
                  bias_grad=G["mlp_head.1.bias"])
        dYc = self.new(2 * B, DIM)
        self.gemm(0, 0, 2 * B, DIM, n, dl2.data_ptr(), n, P["mlp_head.1.weight"], DIM, dYc.data_ptr(), DIM)
        dC = self.new(2 * B, DIM)
        L.vc_layernorm_bwd(2 * B, DIM, dYc.data_ptr(), DIM, sv["C"].data_ptr(), DIM, P["mlp_head.0.weight"],
                           sv["mu"].data_ptr(), sv["rs"].data_ptr(), dC.data_ptr(), DIM, 0.0, G["mlp_head.0.weight"],
                           G["mlp_head.0.bias"], 0.0, scr, ns, s)
        # cross-token step, then the encoder layers
        st = B * T * DIM
        dX1 = self.new(2, B, T, DIM)
        L.vc_hct_ctattn_bwd(B, T, sv["X1"].data_ptr(), st, self.W["ct0"], self.W["ct1"], *sv["cp"], ptr(sv["mk_c"]),
                            dC.data_ptr(), dX1.data_ptr(), st, GW["ct0"], GW["ct1"], scr, ns, s)
        dX0 = self.new(2, B, T, DIM)
        L.vc_hct_encoder_bwd(B, T, sv["X0"].data_ptr(), st, self.W["enc0"], self.W["enc1"], *sv["ep"], ptr(sv["mk_e"]),
                             dX1.data_ptr(), st, dX0.data_ptr(), st, GW["enc0"], GW["enc1"], scr, ns, s)
        # tokeniser: the HSI call leaves its partial rows, the LiDAR call reduces both sources' together
        dz2, dzl = self.new(M2, DIM), self.new(M1, DIM)
        L.vc_hct_tokpool_bwd(B, H2 * H2, Lt, sv["z2"].data_ptr(), DIM, P["token_wA"], P["token_wV"],
                             sv["AH"].data_ptr(), sv["UH"].data_ptr(), dX0[0].data_ptr(), ptr(sv["mk_h"]), sv["pe"],
                             dz2.data_ptr(), DIM, scr, ns, 0, None, None, None, None, s)
        L.vc_hct_tokpool_bwd(B, H1 * H1, Lt, sv["zl"].data_ptr(), DIM, P["token_wA"], P["token_wV"],
                             sv["AL"].data_ptr(), sv["UL"].data_ptr(), dX0[1].data_ptr(), ptr(sv["mk_l"]), sv["pe"],
                             dzl.data_ptr(), DIM, scr, ns, B, G["token_wA"], G["token_wV"], G["pos_embedding"],
                             G["cls_token"], s)
        # LiDAR branch: BatchNorm + ReLU, conv (x2 is data: no input gradient)
        dyl = self.new(M1, DIM)
        L.vc_bn_bwd_relu_ex(tr, M1, DIM, dzl.data_ptr(), DIM, sv["yl"].data_ptr(), DIM, sv["meanl"].data_ptr(),
                            sv["invl"].data_ptr(), P["conv2d_features2.1.weight"], P["conv2d_features2.1.bias"],
                            dyl.data_ptr(), DIM, 0.0, G["conv2d_features2.1.weight"], G["conv2d_features2.1.bias"], 0.0,
                            scr, ns, self.cnt, N_COUNTERS, s)
        L.vc_conv3x3_tap_wgrad_oihw(B, Pp, Pp, m.in_channels, DIM, 0, sv["x2r"].data_ptr(), sv["ld2"], dyl.data_ptr(),
                                    DIM, G["conv2d_features2.0.weight"], G["conv2d_features2.0.bias"], scr, ns, s)
        # HSI branch: BatchNorm2d + ReLU, conv 8 -> 64, BatchNorm3d + ReLU, conv 3 -> 8 (x1 is data)
        dy2 = self.new(M2, DIM)
        L.vc_bn_bwd_relu_ex(tr, M2, DIM, dz2.data_ptr(), DIM, sv["y2"].data_ptr(), DIM, sv["mean2"].data_ptr(),
                            sv["inv2"].data_ptr(), P["conv2d_features.1.weight"], P["conv2d_features.1.bias"],
                            dy2.data_ptr(), DIM, 0.0, G["conv2d_features.1.weight"], G["conv2d_features.1.bias"], 0.0,
                            scr, ns, self.cnt, N_COUNTERS, s)
        L.vc_conv3x3_tap_wgrad_oihw(B, H1, H1, 8, DIM, 0, sv["z3"].data_ptr(), 8, dy2.data_ptr(), DIM,
                                    G["conv2d_features.0.weight"], G["conv2d_features.0.bias"], scr, ns, s)
        dz3 = self.new(M1, 8)
        L.vc_conv3x3_tap_dgrad(B, H1, H1, 8, DIM, 0, dy2.data_ptr(), DIM, sv["wt2"].data_ptr(), 0.0, dz3.data_ptr(), 8,
                               scr, ns, s)
        dy3 = self.new(M1, 8)
        L.vc_bn_bwd_relu_ex(tr, M1, 8, dz3.data_ptr(), 8, sv["y3"].data_ptr(), 8, sv["mean3"].data_ptr(),
                            sv["inv3"].data_ptr(), P["conv3d_features.1.weight"], P["conv3d_features.1.bias"],
                            dy3.data_ptr(), 8, 0.0, G["conv3d_features.1.weight"], G["conv3d_features.1.bias"], 0.0,
                            scr, ns, self.cnt, N_COUNTERS, s)
        L.vc_conv3x3_tap_wgrad_oihw(B, Pp, Pp, 3, 8, 0, sv["x1r"].data_ptr(), sv["ld1"], dy3.data_ptr(), 8,
                                    G["conv3d_features.0.weight"], G["conv3d_features.0.bias"], scr, ns, s)
        self.sv = {}
        return grad
