"""MHST comparison model (the multi-head-select pooling transformer, HSI + LiDAR) on the MI355X path.

Reference: `model/compare_method/MHST/` (`MHST.py` `MHST` :250-325, `HSI_Encoder` :57-119, `LiDAR_Encoder` :23-54,
`Classifier` :122-147, `Transformer` :220-247; `HSPT.py` `HeadSelectPoolTransformer` :390-443, `StepPoolViTBlock`
:324-387, `PoolAttention` :142-290, `DynaLinear` :66-139, `HeadSelectBlock` :38-63, `_gumbel_sigmoid` :7-30;
`Pooling.py` `attn_pool`; `PyConv2D.py`), built by `model_utils.py:314-335` (patch 8, width 64, 5 encoder layers of
4 heads, 8 head-select blocks of 16 heads, tau 5, dropout 0.1, AdamW lr 8e-4).  The module keeps the reference's
parameter tree, creation order and initialisers, so `state_dict()` has the reference's 338 keys, `.pth` files
interchange and the same `torch.manual_seed` draws the same initial values.  The reference's only `timm` import
(`DropPath`) is never instantiated at drop_path_rate 0; nothing here needs it.

Forward and backward are one hand-written program of HIP kernels over channels-last rows: the
3-D stage and every pyramidal convolution through `vc_mhst_conv_*` (one grouped 3-D family; the grouped 2-D convs over
the `(c d)` reshape run on the 3-D rows as they are) except the 3x3x3 conv, an implicit GEMM on the MFMA
(`vc_mhst_conv3_*`), BatchNorm + ReLU through `vc_bn_*_ex`, the 1x1 convs and every
Linear through `vc_gemm_ex`, `vc_maxpool2_*`, `vc_mhst_embed_*`, the five `en_transformer` layers on S2EFT's kernels
(`vc_s2eft_attn_*`, `vc_gelu_*`), then per head-select block the fused chain gate -> head mask -> pooling -> attention ->
head mask (`vc_mhst_hsattn_*`, one block per (sample, head) with the head's rows and probabilities in LDS) between the
q | k | v and proj GEMMs, `vc_mhst_headmask_*` on the MLP's input, and `vc_mhst_tail_*` for the mixture of the two
softmax outputs.  The output is
that mixture of probabilities, as in the reference (`CrossEntropyLoss` and `test()` receive it).

Randomness: the dropout masks (`vc_dropout_fwd`, and the attention probabilities' inside `vc_mhst_hsattn_fwd`) and the
gates' logistic noise come from the package's counter hash, seeded by `program.seed_dropout` (the device-side step seed
under `seeds.attach`).  `forward(hsi, lidar, gate_noise=[depth, B, 16])` takes the noise (g1 - g2 of the reference's two
Gumbel draws) from the caller instead; the program keeps what it used in `noise`, the decisions in `sel`.

`conv` (keyword only, `set_conv`; the positional signature and the state_dict are the reference's): "direct", the
default and the recorded program, or "mfma": every pyramidal site whose shape `vc_mhst_pconv_ok` accepts
(`hsi_encoder.conv4`, `lidar_encoder.conv2`, `pyconv_classifier.conv1`) runs forward, data and weight gradient through
`vc_mhst_pconv_*`, exact-fp32 implicit GEMMs on the MFMA, in train, eval and `test()`; the strided
`hsi_encoder.conv1`, the spectral convs and `lidar_encoder.conv1` stay on `vc_mhst_conv_*`.  "mfma_all" is "mfma" plus the
front of the HSI encoder on the MFMA: `hsi_encoder.conv1` through `vc_mhst_conv1_fwd / _wgrad` and the four spectral
convolutions as one convolution, `vc_mhst_sconv_fwd` forward and one `vc_mhst_sconv_wgrad` then one `vc_mhst_sconv_dgrad`
backward; only `lidar_encoder.conv1` (1 to 3 input channels) stays on `vc_mhst_conv_*`.

The patch side is 8 (`encoder_embedding` is Linear(16, 64) and `PoolAttention.hw_shape` (8, 8)); any HSI and LiDAR
band count >= 1.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import program, seeds
from ._lib import lib
from .flat import F32, FlatParams

LN_EPS = 1e-5
DIM = 64
T = 65
HS_HEADS = 16
EN_HEADS, EN_DIM_HEAD = program.ATTN_HEADS, program.ATTN_DIM_HEAD
PATCH = 8
EMBED_PART = 1156   # VC_MHST_EMBED_PART
POOL_FLOATS = 132   # VC_MHST_POOL_FLOATS
NCLS_MAX = 256      # vc_mhst_tail_*
PY_KERNELS = (3, 5, 7, 9)
SPECTRAL_TAPS = (1, 3, 5, 11)
GATE_SITE = 100000  # the gates' seed sites start here, clear of the dropout sites
# en_transformer (MHST.py:220-247) as program.encoder_fwd / _bwd take it: pre-norm layers over the 65 tokens
ENCODER = dict(prefix="en_transformer", T=T, D=DIM, ff="mlp", site="en")


# ---------------------------------------------------------------- parameter tree (reference names)
def _conv(cin, cout, k, groups):
    return nn.Conv2d(cin, cout, kernel_size=k, stride=1, padding=k // 2, groups=groups, bias=False)


class PyConv4(nn.Module):
    def __init__(self, inplans, planes, groups):
        super().__init__()
        for i, (k, g) in enumerate(zip(PY_KERNELS, groups)):
            setattr(self, f"conv2_{i + 1}", _conv(inplans, planes // 4, k, g))


class PyConv2(nn.Module):
    def __init__(self, inplans, planes, groups):
        super().__init__()
        for i, (k, g) in enumerate(zip((3, 5), groups)):
            setattr(self, f"conv2_{i + 1}", _conv(inplans, planes // 2, k, g))


class LiDAR_Encoder(nn.Module):
    def __init__(self, in_channels=1, out_channels=64):
        super().__init__()
        self.conv1 = PyConv4(in_channels, 32, (1, 1, 1, 1))
        self.bn1 = nn.BatchNorm2d(32)
        self.conv2 = PyConv4(32, out_channels, (1, 1, 1, 1))
        self.bn2 = nn.BatchNorm2d(out_channels)
        self.conv3 = nn.Conv2d(out_channels, out_channels, kernel_size=1)
        self.bn3 = nn.BatchNorm2d(out_channels)


class HSI_Encoder(nn.Module):
    def __init__(self, in_depth_3d=144):
        super().__init__()
        self.conv1 = nn.Conv3d(1, 16, kernel_size=(11, 3, 3), stride=(3, 1, 1), padding=(5, 1, 1))
        self.bn1 = nn.BatchNorm3d(16)
        for i, k in enumerate(SPECTRAL_TAPS):
            setattr(self, f"conv2_{i + 1}", nn.Conv3d(16, 4, kernel_size=(k, 1, 1), padding=(k // 2, 0, 0)))
        self.bn2 = nn.BatchNorm3d(16)
        self.conv3 = nn.Conv3d(16, 16, kernel_size=(3, 3, 3), padding=(1, 1, 1))
        self.bn3 = nn.BatchNorm3d(16)
        self.in_channels_2d = int((in_depth_3d + 2) / 3) * 16
        self.conv4 = PyConv4(self.in_channels_2d, 64, (1, 2, 4, 8))
        self.bn4 = nn.BatchNorm2d(64)
        self.conv5 = nn.Conv2d(64, 64, kernel_size=1)
        self.bn5 = nn.BatchNorm2d(64)


class Classifier(nn.Module):
    def __init__(self, classes):
        super().__init__()
        self.conv1 = PyConv2(64, 32, (2, 2))
        self.bn1 = nn.BatchNorm2d(32)
        self.conv2 = nn.Sequential(nn.Conv2d(32, classes, 1))


class Residual(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn


class PreNorm(nn.Module):
    def __init__(self, dim, fn):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.fn = fn


class FeedForward(nn.Module):
    def __init__(self, dim, hidden_dim, dropout=0.):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(dim, hidden_dim), nn.GELU(), nn.Dropout(dropout), nn.Linear(hidden_dim, dim),
                                 nn.Dropout(dropout))


class Attention(nn.Module):
    def __init__(self, dim, heads, dim_head, dropout):
        super().__init__()
        inner = dim_head * heads
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.to_qkv = nn.Linear(dim, inner * 3, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, dim), nn.Dropout(dropout))


class Transformer(nn.Module):
    def __init__(self, dim, depth, heads, dim_head, mlp_head, dropout):
        super().__init__()
        self.layers = nn.ModuleList([])
        for _ in range(depth):
            self.layers.append(nn.ModuleList([
                Residual(PreNorm(dim, Attention(dim, heads=heads, dim_head=dim_head, dropout=dropout))),
                Residual(PreNorm(dim, FeedForward(dim, mlp_head, dropout=dropout)))]))


class HeadSelectBlock(nn.Module):
    def __init__(self, dim_in, num_heads, tau=5):
        super().__init__()
        self.mlp_head = nn.Linear(dim_in, num_heads, bias=True)
        self.tau = tau


class PoolAttention(nn.Module):
    def __init__(self, dim, num_heads, attn_drop=0., proj_drop=0.):
        super().__init__()
        hd = dim // num_heads
        self.query = nn.Linear(dim, dim, bias=False)
        self.key = nn.Linear(dim, dim, bias=False)
        self.value = nn.Linear(dim, dim, bias=False)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        for n in "qkv":
            setattr(self, "pool_" + n, nn.Conv2d(hd, hd, (3, 3), stride=(1, 1), padding=(1, 1), groups=hd, bias=False))
            setattr(self, "norm_" + n, nn.LayerNorm(hd))


class MlpBlock(nn.Module):
    def __init__(self, in_features, hidden_features, drop=0.):
        super().__init__()
        self.act = nn.GELU()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, in_features)
        self.drop = nn.Dropout(drop)


class StepPoolViTBlock(nn.Module):
    def __init__(self, dim, num_heads, head_tau, drop, attn_drop, mlp_ratio):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn = PoolAttention(dim, num_heads, attn_drop=attn_drop, proj_drop=drop)
        self.drop_path = nn.Identity()
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = MlpBlock(dim, int(dim * mlp_ratio), drop=drop)
        self.head_select = HeadSelectBlock(dim, num_heads, tau=head_tau)


class HeadSelectPoolTransformer(nn.Module):
    def __init__(self, dim, depth, num_heads, head_tau, drop, attn_drop, mlp_ratio):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.blocks = nn.ModuleList([StepPoolViTBlock(dim, num_heads, head_tau, drop, attn_drop, mlp_ratio)
                                     for _ in range(depth)])


class MHST(FlatParams, nn.Module):
    """Same constructor as the reference `MHST` (MHST.py:251-259); forward(hsi [B,l1,8,8], lidar [B,l2,8,8]) ->
    the mixture of the two classifiers' probabilities [B, num_classes]."""

    draws_noise = True   # the head gates draw from the step seed even with every dropout at 0 (seeds.has_dropout)

    def __init__(self, l1, l2, patch_size, num_patches, num_classes, encoder_embed_dim, en_depth, en_heads, mlp_dim,
                 dim_head=16, dropout=0., emb_dropout=0., coefficient_hsi=0.5, coefficient_vit=0.5, hsp_vit_depth=12,
                 hsp_vit_num_heads=16, vit_qkv_bias=True, use_head_select=True, head_tau=5, mlp_ratio=4.,
                 attnproj_mlp_drop=0., attn_drop=0., *, conv="direct"):
        super().__init__()
        self.conv = _check_conv(conv)
        _check_supported(l1, l2, patch_size, num_classes, encoder_embed_dim, en_depth, en_heads, mlp_dim, dim_head,
                         dropout, emb_dropout, hsp_vit_depth, hsp_vit_num_heads, vit_qkv_bias, use_head_select, head_tau,
                         mlp_ratio, attnproj_mlp_drop, attn_drop)
        self.num_patches, self.patch_size = num_patches, patch_size
        self.l1, self.l2, self.ncls = l1, l2, num_classes
        self.en_depth, self.hs_depth, self.mlp_dim = en_depth, hsp_vit_depth, mlp_dim
        self.hs_hidden = int(DIM * mlp_ratio)
        self.head_tau = float(head_tau)
        # creation order = the reference's, so the default initialisation draws the same numbers
        self.hsi_encoder = HSI_Encoder(in_depth_3d=l1)
        self.lidar_encoder = LiDAR_Encoder(in_channels=l2, out_channels=64)
        self.weight_hsi = nn.Parameter(torch.Tensor([coefficient_hsi]))
        self.weight_lidar = nn.Parameter(torch.Tensor([1 - coefficient_hsi]))
        self.encoder_embedding = nn.Linear((patch_size // 2) ** 2, patch_size ** 2)
        self.cls_token = nn.Parameter(torch.randn(1, 1, encoder_embed_dim))
        self.dropout = nn.Dropout(emb_dropout)
        self.encoder_pos_embed = nn.Parameter(torch.randn(1, patch_size ** 2 + 1, encoder_embed_dim))
        self.en_transformer = Transformer(encoder_embed_dim, en_depth, en_heads, dim_head, mlp_dim, dropout)
        self.HeadSelectViT = HeadSelectPoolTransformer(encoder_embed_dim, hsp_vit_depth, hsp_vit_num_heads, head_tau,
                                                       attnproj_mlp_drop, attn_drop, mlp_ratio)
        self.to_latent = nn.Identity()
        self.pyconv_classifier = Classifier(num_classes)
        self.mlp_head = nn.Sequential(nn.LayerNorm(encoder_embed_dim), nn.Linear(encoder_embed_dim, num_classes))
        self.vit_cls_coefficient = nn.Parameter(torch.Tensor([coefficient_vit]))
        self.cnn_cls_coefficient = nn.Parameter(torch.Tensor([1 - coefficient_vit]))
        self._build_flat()
        _check_packed(self)

    def set_conv(self, conv: str):
        """The family behind the convolutions: "direct" (`vc_mhst_conv_*`), "mfma" (`vc_mhst_pconv_*` at every pyramidal
        site whose shape `vc_mhst_pconv_ok` accepts) or "mfma_all" ("mfma" plus `vc_mhst_conv1_*` at `hsi_encoder.conv1`
        and `vc_mhst_sconv_*` for the four spectral convolutions).  Every forward builds its program from the current
        value; a TrainStepper's captured graphs are bound to the mode they recorded and are dropped when it changes."""
        self.conv = _check_conv(conv)
        return self

    def forward(self, hsi: torch.Tensor, lidar: torch.Tensor, gate_noise: torch.Tensor = None) -> torch.Tensor:
        if hsi.device.type != "cuda" or lidar.device.type != "cuda":
            raise RuntimeError("MHST MI355X path: inputs must be on a ROCm (cuda) device; no CPU fallback")
        if hsi.dim() != 4 or hsi.shape[1] != self.l1:
            raise RuntimeError(f"expected hsi [B, {self.l1}, {PATCH}, {PATCH}], got {list(hsi.shape)}")
        if tuple(hsi.shape[2:]) != (PATCH, PATCH):
            raise RuntimeError(f"MHST MI355X path: the patch side must be {PATCH}, got {list(hsi.shape[2:])}")
        if lidar.dim() != 4 or tuple(lidar.shape) != (hsi.shape[0], self.l2, PATCH, PATCH):
            raise RuntimeError(f"expected lidar [B, {self.l2}, {PATCH}, {PATCH}] matching hsi, got {list(lidar.shape)}")
        if hsi.shape[0] < 1:
            raise RuntimeError("empty batch")
        if gate_noise is not None:
            if tuple(gate_noise.shape) != (self.hs_depth, hsi.shape[0], HS_HEADS):
                raise RuntimeError(f"expected gate_noise [{self.hs_depth}, B, {HS_HEADS}], got {list(gate_noise.shape)}")
            gate_noise = gate_noise.detach().to(device=hsi.device, dtype=torch.float32).contiguous()
        hsi = hsi.detach().to(torch.float32).contiguous()
        lidar = lidar.detach().to(torch.float32).contiguous()
        if gate_noise is None:
            return program.run(self, _Program, hsi, lidar)
        return program.run(self, _Program, hsi, lidar, gate_noise)


CONV_MODES = ("direct", "mfma", "mfma_all")


def _check_conv(conv):
    if conv not in CONV_MODES:
        raise ValueError(f"MHST: conv must be one of {CONV_MODES}, got {conv!r}")
    return conv


def _check_supported(l1, l2, patch_size, num_classes, dim, en_depth, en_heads, mlp_dim, dim_head, dropout, emb_dropout,
                     hs_depth, hs_heads, qkv_bias, use_head_select, head_tau, mlp_ratio, drop, attn_drop):
    """reject what a kernel cannot take, at construction"""
    pre = "MHST MI355X path: "
    if patch_size != PATCH:
        raise ValueError(f"{pre}patch_size must be {PATCH} (encoder_embedding and the pooling grid), got {patch_size}")
    if dim != DIM:
        raise ValueError(f"{pre}encoder_embed_dim must be {DIM}, got {dim}")
    if (en_heads, dim_head) != (EN_HEADS, EN_DIM_HEAD):
        raise ValueError(f"{pre}en_heads, dim_head must be {(EN_HEADS, EN_DIM_HEAD)} (vc_s2eft_attn_*), got "
                         f"{(en_heads, dim_head)}")
    if hs_heads != HS_HEADS:
        raise ValueError(f"{pre}hsp_vit_num_heads must be {HS_HEADS} (vc_mhst_attn_*), got {hs_heads}")
    if qkv_bias or not use_head_select:
        raise ValueError(f"{pre}vit_qkv_bias must be False and use_head_select True (the registry's configuration)")
    if l1 < 1 or l2 < 1 or not 1 <= num_classes <= NCLS_MAX:
        raise ValueError(f"MHST: band counts must be positive and num_classes in 1..{NCLS_MAX}")
    if en_depth < 0 or hs_depth < 1 or mlp_dim < 1 or int(DIM * mlp_ratio) < 1 or not head_tau > 0:
        raise ValueError("MHST: en_depth >= 0, hsp_vit_depth >= 1, mlp_dim >= 1, mlp_ratio and head_tau positive")
    if not all(0.0 <= p < 1.0 for p in (dropout, emb_dropout, drop, attn_drop)):
        raise ValueError("MHST: every dropout probability must be in [0, 1)")


def _check_packed(m):
    """a block's query | key | value weights (one [192, 64] GEMM operand) and its pooling parameters (vc_mhst_pool_*'s
    132 floats) must be contiguous in the flat buffer, in module order"""
    for i in range(m.hs_depth):
        a = f"HeadSelectViT.blocks.{i}.attn."
        o = m._poff[a + "query.weight"]
        if (m._poff[a + "key.weight"], m._poff[a + "value.weight"]) != (o + DIM * DIM, o + 2 * DIM * DIM):
            raise RuntimeError("MHST: query / key / value weights are not contiguous in the flat buffer")
        o = m._poff[a + "pool_q.weight"]
        for n in "qkv":
            if (m._poff[a + f"pool_{n}.weight"], m._poff[a + f"norm_{n}.weight"], m._poff[a + f"norm_{n}.bias"]) != \
                    (o, o + 36, o + 40):
                raise RuntimeError("MHST: the pooling parameters are not contiguous in the flat buffer")
            o += 44


class _Program(program.Program):
    NAME = "MHST"
    LN_EPS = LN_EPS
    D = DIM

    def __init__(self, m: MHST, needs_grad, x1, x2, gate_noise=None):
        super().__init__(lib(), m, needs_grad, x1, x2)
        self.x1, self.x2 = x1, x2
        self.D1 = (m.l1 + 2) // 3
        part = self.B * max(EMBED_PART, m.ncls * 33 + 2)
        # ONE workspace for the GEMMs' split-K slabs, vc_colsum / BatchNorm partials and the 3x3x3 weight gradient's
        # per-wave partials: every launch of the program is on one stream, in order, and each kernel has consumed its
        # partials when it ends, so no two users overlap.  A second stream would need a workspace of its own.
        self.mfma = m.conv in ("mfma", "mfma_all")
        self.front = m.conv == "mfma_all"   # hsi_encoder.conv1 and the spectral convs on the MFMA too
        pws = max(self.pconv_ws(shp) for kind in self.shapes().values()
                  for shp in (kind if isinstance(kind, list) else [kind])) if self.mfma else 0
        if self.front:
            pws = max(pws, self.L.vc_mhst_conv1_ws_floats(self.B, m.l1), self.L.vc_mhst_sconv_ws_floats(self.B, self.D1))
        self.scratch(max(1 << 22, part, self.L.vc_mhst_conv3_wgrad_ws_floats(self.B, self.D1), pws), grow=True)
        self.noise_in = gate_noise
        self.seed_dropout(self.train)

    # ------------------------------------------------------------ helpers
    @staticmethod
    def pconv_args(shape):
        """(D, C, O, G, KS) of a conv shape that is a whole-depth convolution on the 8 x 8 map, else None"""
        D, H, W, C, O, G, KD, KS, sd, pd, Dout = shape
        return (D, C, O, G, KS) if (H, W, KD, sd, pd, Dout) == (8, 8, D, 1, 0, 1) else None

    def pconv(self, shape, ldx, ldy):
        """vc_mhst_pconv_*'s shape arguments where the model runs in "mfma" mode and the family takes the site"""
        a = self.pconv_args(shape) if self.mfma else None
        return a if a is not None and self.L.vc_mhst_pconv_ok(*a, ldx, ldy) else None

    def pconv_ws(self, shape):
        a = self.pconv_args(shape)
        if a is None or not self.L.vc_mhst_pconv_ok(*a, a[1] + (-a[1] % 4), a[2] + (-a[2] % 4)):
            return 0
        return self.L.vc_mhst_pconv_ws_floats(self.B, *a)

    def conv(self, shape, x, ldx, w, bias, y, ycol, ldy):
        a = self.pconv(shape, ldx, ldy)
        if a is not None:
            self.L.vc_mhst_pconv_fwd(self.B, *a, x.data_ptr(), ldx, self.P[w], self.P[bias] if bias else None,
                                     y.data_ptr() + F32 * ycol, ldy, self.scr.data_ptr(), self.SCRATCH, self.s)
            return
        self.L.vc_mhst_conv_fwd(self.B, *shape, x.data_ptr(), ldx, self.P[w], self.P[bias] if bias else None,
                                y.data_ptr() + F32 * ycol, ldy, self.s)

    def conv_bwd(self, shape, x, ldx, w, bias, dy, ycol, ldy, dx=None, beta=0.0):
        L = self.L
        a = self.pconv(shape, ldx, ldy)
        if a is not None:
            scr, ns = self.scr.data_ptr(), self.SCRATCH
            L.vc_mhst_pconv_wgrad(self.B, *a, x.data_ptr(), ldx, dy.data_ptr() + F32 * ycol, ldy, self.G[w],
                                  self.G[bias] if bias else None, scr, ns, self.s)
            if dx is not None:
                L.vc_mhst_pconv_dgrad(self.B, *a, dy.data_ptr() + F32 * ycol, ldy, self.P[w], dx.data_ptr(), ldx, beta,
                                      scr, ns, self.s)
            return
        L.vc_mhst_conv_wgrad(self.B, *shape, x.data_ptr(), ldx, dy.data_ptr() + F32 * ycol, ldy, self.G[w],
                             self.G[bias] if bias else None, self.s)
        if dx is not None:
            L.vc_mhst_conv_dgrad(self.B, *shape, dy.data_ptr() + F32 * ycol, ldy, self.P[w], dx.data_ptr(), ldx, beta,
                                 self.s)

    # the conv shapes (D, H, W, C, O, G, KD, KS, sd, pd, Dout) of the model
    def shapes(self):
        m, D1 = self.m, self.D1
        return {
            "h1": (m.l1, 8, 8, 1, 16, 1, 11, 3, 3, 5, D1),
            "h2": [(D1, 8, 8, 16, 4, 1, k, 1, 1, k // 2, D1) for k in SPECTRAL_TAPS],
            "h3": (D1, 8, 8, 16, 16, 1, 3, 3, 1, 1, D1),
            "h4": [(D1, 8, 8, 16, 16, g, D1, k, 1, 0, 1) for k, g in zip(PY_KERNELS, (1, 2, 4, 8))],
            "l1": [(1, 8, 8, m.l2, 8, 1, 1, k, 1, 0, 1) for k in PY_KERNELS],
            "l2": [(1, 8, 8, 32, 16, 1, 1, k, 1, 0, 1) for k in PY_KERNELS],
            "c1": [(1, 8, 8, 64, 16, 2, 1, k, 1, 0, 1) for k in (3, 5)],
        }

    # ------------------------------------------------------------ forward
    def _forward(self):
        m, L, B, P, s = self.m, self.L, self.B, self.P, self.s
        D1 = self.D1
        sh = self.shapes()
        sv = self.sv = {}
        M3, M2 = B * D1 * 64, B * 64
        he, le = m.hsi_encoder, m.lidar_encoder
        # HSI encoder (MHST.py:93-119): x1 [B, l1, 8, 8] is the 3-D rows (b, d, h, w) of one channel
        y1 = self.new(M3, 16)
        scr, ns = self.scr.data_ptr(), self.SCRATCH
        if self.front:
            L.vc_mhst_conv1_fwd(B, m.l1, self.x1.data_ptr(), P["hsi_encoder.conv1.weight"], P["hsi_encoder.conv1.bias"],
                                y1.data_ptr(), 16, scr, ns, s)
        else:
            self.conv(sh["h1"], self.x1, 1, "hsi_encoder.conv1.weight", "hsi_encoder.conv1.bias", y1, 0, 16)
        z1, mean1, inv1 = self.bn("hsi_encoder.bn1", he.bn1, y1, M3, 16)
        y2 = self.new(M3, 16)
        spectral = [f"hsi_encoder.conv2_{i + 1}" for i in range(len(SPECTRAL_TAPS))]
        if self.front:   # the four spectral convs as one convolution, one launch
            L.vc_mhst_sconv_fwd(B, D1, z1.data_ptr(), 16, *(P[pf + ".weight"] for pf in spectral),
                                *(P[pf + ".bias"] for pf in spectral), y2.data_ptr(), 16, scr, ns, s)
        else:
            for i, (pf, shp) in enumerate(zip(spectral, sh["h2"])):
                self.conv(shp, z1, 16, pf + ".weight", pf + ".bias", y2, 4 * i, 16)
        z2, mean2, inv2 = self.bn("hsi_encoder.bn2", he.bn2, y2, M3, 16)
        y3 = self.new(M3, 16)
        L.vc_mhst_conv3_fwd(B, D1, z2.data_ptr(), 16, P["hsi_encoder.conv3.weight"], P["hsi_encoder.conv3.bias"],
                            y3.data_ptr(), 16, s)   # the 3x3x3 conv: implicit GEMM on the MFMA
        z3, mean3, inv3 = self.bn("hsi_encoder.bn3", he.bn3, y3, M3, 16)
        y4 = self.new(M2, 64)
        for i, shp in enumerate(sh["h4"]):   # the (c d) reshape is the 3-D rows as they are: KD = D1
            self.conv(shp, z3, 16, f"hsi_encoder.conv4.conv2_{i + 1}.weight", None, y4, 16 * i, 64)
        z4, mean4, inv4 = self.bn("hsi_encoder.bn4", he.bn4, y4, M2, 64)
        y5 = self.linear(z4, M2, 64, 64, "hsi_encoder.conv5")
        z5, mean5, inv5 = self.bn("hsi_encoder.bn5", he.bn5, y5, M2, 64)
        ph, argh = self.new(B * 16, 64), self.bytes(B * 16, 64)
        L.vc_maxpool2_fwd(B, 8, 8, 64, z5.data_ptr(), 64, ph.data_ptr(), argh.data_ptr(), s)
        # LiDAR encoder (:40-54)
        x2r, ld2 = self.rows(self.x2, m.l2, 64)
        yl1 = self.new(M2, 32)
        for i, shp in enumerate(sh["l1"]):
            self.conv(shp, x2r, ld2, f"lidar_encoder.conv1.conv2_{i + 1}.weight", None, yl1, 8 * i, 32)
        zl1, meanl1, invl1 = self.bn("lidar_encoder.bn1", le.bn1, yl1, M2, 32)
        yl2 = self.new(M2, 64)
        for i, shp in enumerate(sh["l2"]):
            self.conv(shp, zl1, 32, f"lidar_encoder.conv2.conv2_{i + 1}.weight", None, yl2, 16 * i, 64)
        zl2, meanl2, invl2 = self.bn("lidar_encoder.bn2", le.bn2, yl2, M2, 64)
        yl3 = self.linear(zl2, M2, 64, 64, "lidar_encoder.conv3")
        zl3, meanl3, invl3 = self.bn("lidar_encoder.bn3", le.bn3, yl3, M2, 64)
        pl, argl = self.new(B * 16, 64), self.bytes(B * 16, 64)
        L.vc_maxpool2_fwd(B, 8, 8, 64, zl3.data_ptr(), 64, pl.data_ptr(), argl.data_ptr(), s)
        # fusion and tokens (:287-301)
        xcnn, Xe = self.new(B * 64, DIM), self.new(B * T, DIM)
        L.vc_mhst_embed_fwd(B, ph.data_ptr(), pl.data_ptr(), P["weight_hsi"], P["weight_lidar"],
                            P["encoder_embedding.weight"], P["encoder_embedding.bias"], P["encoder_pos_embed"],
                            P["cls_token"], xcnn.data_ptr(), Xe.data_ptr(), s)
        self.pe = self.drop_p(m.dropout)
        X = self.dropped("emb", Xe, None, B * T * DIM, self.pe, DIM)
        sv.update(y1=y1, z1=z1, mean1=mean1, inv1=inv1, y2=y2, z2=z2, mean2=mean2, inv2=inv2, y3=y3, z3=z3, mean3=mean3,
                  inv3=inv3, y4=y4, z4=z4, mean4=mean4, inv4=inv4, y5=y5, mean5=mean5, inv5=inv5, ph=ph, argh=argh,
                  x2r=x2r, ld2=ld2, yl1=yl1, zl1=zl1, meanl1=meanl1, invl1=invl1, yl2=yl2, zl2=zl2, meanl2=meanl2,
                  invl2=invl2, yl3=yl3, meanl3=meanl3, invl3=invl3, pl=pl, argl=argl, xcnn=xcnn)
        X, self.enc = self.encoder_fwd(X, layers=m.en_transformer.layers, hidden=m.mlp_dim, **ENCODER)
        X = self.headselect_fwd(X)
        # classifier (:308-319): the transformer's cls row through HeadSelectViT.norm and mlp_head ...
        Yn, mun, rsn = self.ln("HeadSelectViT.norm", X.data_ptr(), B, T * DIM)
        Yc, muc, rsc = self.ln("mlp_head.0", Yn.data_ptr(), B, DIM)
        lg1 = self.linear(Yc, B, DIM, m.ncls, "mlp_head.1")
        # ... and the CNN classifier on x_cnn as a [B, 64, 8, 8] map (tokens are the pixels, the width the channels)
        yc = self.new(M2, 32)
        for i, shp in enumerate(sh["c1"]):
            self.conv(shp, xcnn, 64, f"pyconv_classifier.conv1.conv2_{i + 1}.weight", None, yc, 16 * i, 32)
        zc, meanc, invc = self.bn("pyconv_classifier.bn1", m.pyconv_classifier.bn1, yc, M2, 32)
        n = m.ncls
        p1, p2, avg, out = self.new(B, n), self.new(B, n), self.new(B, 32), self.new(B, n)
        L.vc_mhst_tail_fwd(B, n, lg1.data_ptr(), zc.data_ptr(), 32, P["pyconv_classifier.conv2.0.weight"],
                           P["pyconv_classifier.conv2.0.bias"], P["vit_cls_coefficient"], P["cnn_cls_coefficient"],
                           p1.data_ptr(), p2.data_ptr(), avg.data_ptr(), out.data_ptr(), s)
        # the ReLU outputs and max-pool taps, kept for whoever audits the decisions (tests: `decisions()`)
        self.dec = dict(relu={"hsi_encoder.bn1": (z1, D1), "hsi_encoder.bn2": (z2, D1), "hsi_encoder.bn3": (z3, D1),
                              "hsi_encoder.bn4": (z4, 0), "hsi_encoder.bn5": (z5, 0), "lidar_encoder.bn1": (zl1, 0),
                              "lidar_encoder.bn2": (zl2, 0), "lidar_encoder.bn3": (zl3, 0),
                              "pyconv_classifier.bn1": (zc, 0)},
                        pool={"hsi": (argh, ph), "lidar": (argl, pl)})
        sv.update(Xlast=X, Yn=Yn, mun=mun, rsn=rsn, Yc=Yc, muc=muc, rsc=rsc, yc=yc, meanc=meanc, invc=invc, p1=p1, p2=p2,
                  avg=avg)
        return out

    def decisions(self):
        """the last forward's ReLU outputs in the reference's layouts ([B, C, 8, 8] or [B, C, D, 8, 8]: the decision is
        `> 0`) and the two max pools' (winning taps, pooled values) as [B, 16, 64], on the CPU"""
        B, relu = self.B, {}
        for k, (z, D) in self.dec["relu"].items():
            C = z.shape[1]
            relu[k] = (z.view(B, D, 8, 8, C).permute(0, 4, 1, 2, 3) if D else z.view(B, 8, 8, C).permute(0, 3, 1, 2)).cpu()
        pool = {k: (a.view(B, 16, 64).cpu(), v.view(B, 16, 64).cpu()) for k, (a, v) in self.dec["pool"].items()}
        return dict(relu=relu, pool=pool)

    def headselect_fwd(self, X):
        """the head-select blocks (HSPT.py:354-387)"""
        m, L, B, P, s = self.m, self.L, self.B, self.P, self.s
        R, Hh = B * T, m.hs_hidden
        ds = self.dseed
        self.hs = []
        self.noise = self.new(m.hs_depth, B, HS_HEADS)
        self.sel = self.new(m.hs_depth, B, HS_HEADS)
        for i in range(m.hs_depth):
            pre = f"HeadSelectViT.blocks.{i}"
            blk = m.HeadSelectViT.blocks[i]
            pp, pj, pm = self.drop_p(blk.attn.attn_drop), self.drop_p(blk.attn.proj_drop), self.drop_p(blk.mlp.drop)
            # LayerNorm, one GEMM for query | key | value, then the fused chain (DynaLinear's masked output rows :110-125,
            # Pooling.py, attention with residual pooling :254-282, proj's masked input columns), one launch: the gate
            # on the cls row (:38-63) is computed by every (sample, head) block for its own head
            Y, mu, rs = self.ln(pre + ".norm1", X.data_ptr(), R, DIM)
            qkv = self.new(R, 3 * DIM)
            self.gemm(0, 1, R, 3 * DIM, DIM, Y.data_ptr(), DIM, P[pre + ".attn.query.weight"], DIM, qkv.data_ptr(),
                      3 * DIM)
            logits, yg = self.new(B, HS_HEADS), self.new(B, HS_HEADS)
            sel, noise = self.sel[i], self.noise[i]
            nin = self.noise_in[i].data_ptr() if self.noise_in is not None else None
            gsite = seeds.SITE_STRIDE * (GATE_SITE + i)
            mk, psite = None, 0
            if pp > 0:
                mk = self.bytes(B, HS_HEADS, T, T)
                psite = seeds.SITE_STRIDE * len(self.masks)
                self.masks[f"hs{i}.prob"] = mk
            am = self.new(R, DIM)
            if ds is not None:
                entry, seed = L.vc_mhst_hsattn_fwd_ds, (ds.cur_ptr, gsite, psite)
            else:
                entry, seed = L.vc_mhst_hsattn_fwd, ((self.seed + gsite) % (1 << 63), (self.seed + psite) % (1 << 63))
            entry(B, X.data_ptr(), T * DIM, P[pre + ".head_select.mlp_head.weight"],
                  P[pre + ".head_select.mlp_head.bias"], nin, 1 if self.train else 0, m.head_tau, *seed, qkv.data_ptr(),
                  P[pre + ".attn.pool_q.weight"], LN_EPS, 0.5, pp, mk.data_ptr() if mk is not None else None,
                  logits.data_ptr(), noise.data_ptr(), yg.data_ptr(), sel.data_ptr(), am.data_ptr(), s)
            pr = self.linear(am, R, DIM, DIM, pre + ".attn.proj")
            X2 = self.dropped(f"hs{i}.proj", pr, X, R * DIM, pj, DIM)
            # masked MLP (:293-321)
            Y2, mu2, rs2 = self.ln(pre + ".norm2", X2.data_ptr(), R, DIM)
            ym = self.new(R, DIM)
            L.vc_mhst_headmask_fwd(B, T, DIM, Y2.data_ptr(), sel.data_ptr(), ym.data_ptr(), s)
            H1 = self.linear(ym, R, DIM, Hh, pre + ".mlp.fc1")
            Gl = self.new(R, Hh)
            L.vc_gelu_fwd(R * Hh, H1.data_ptr(), Gl.data_ptr(), s)
            Gd = self.dropped(f"hs{i}.fc1", Gl, None, R * Hh, pm, Hh)
            F2 = self.linear(Gd, R, Hh, DIM, pre + ".mlp.fc2")
            X3 = self.dropped(f"hs{i}.fc2", F2, X2, R * DIM, pm, DIM)
            self.hs.append(dict(X=X, yg=yg, sel=sel, Y=Y, mu=mu, rs=rs, qkv=qkv, mk=mk, am=am, X2=X2, Y2=Y2, mu2=mu2,
                                rs2=rs2, ym=ym, H1=H1, Gd=Gd, pp=pp, pj=pj, pm=pm))
            X = X3
        return X

    # ------------------------------------------------------------ backward
    def backward(self, dout):
        """the flat gradient of every parameter, each written once"""
        m, L, B, P, s = self.m, self.L, self.B, self.P, self.s
        D1 = self.D1
        sh = self.shapes()
        sv = self.sv
        M3, M2 = B * D1 * 64, B * 64
        n = m.ncls
        grad = self.new_grad()
        G = self.G
        # tail
        dlg1, dzc = self.new(B, n), self.new(M2, 32)
        wt = n * 33 + 2
        part = self.new(B, wt)
        L.vc_mhst_tail_bwd(B, n, dout.data_ptr(), sv["p1"].data_ptr(), sv["p2"].data_ptr(), sv["avg"].data_ptr(),
                           P["pyconv_classifier.conv2.0.weight"], P["vit_cls_coefficient"], P["cnn_cls_coefficient"],
                           dlg1.data_ptr(), dzc.data_ptr(), 32, part.data_ptr(), s)
        self.reduce_part(part, wt, 0, n * 32, G["pyconv_classifier.conv2.0.weight"])
        self.reduce_part(part, wt, n * 32, n, G["pyconv_classifier.conv2.0.bias"])
        self.reduce_part(part, wt, n * 33, 1, G["vit_cls_coefficient"])
        self.reduce_part(part, wt, n * 33 + 1, 1, G["cnn_cls_coefficient"])
        # CNN classifier -> dxcnn
        dyc = self.bn_bwd("pyconv_classifier.bn1", dzc, sv["yc"], sv["meanc"], sv["invc"], M2, 32)
        dxcnn = self.new(M2, DIM)
        for i, shp in enumerate(sh["c1"]):
            self.conv_bwd(shp, sv["xcnn"], 64, f"pyconv_classifier.conv1.conv2_{i + 1}.weight", None, dyc, 16 * i, 32,
                          dxcnn, 1.0 if i else 0.0)
        # transformer head: mlp_head, HeadSelectViT.norm on the cls rows; every other row of dX starts at zero
        dYc = self.linear_bwd(dlg1, sv["Yc"], B, DIM, n, "mlp_head.1")
        dYn = self.new(B, DIM)
        self.ln_bwd("mlp_head.0", dYc, sv["Yn"].data_ptr(), DIM, sv["muc"], sv["rsc"], B, DIM, dYn.data_ptr(), DIM, 0.0)
        dX = self.new(B * T, DIM)
        L.vc_fill(B * T * DIM, dX.data_ptr(), 0.0, s)
        self.ln_bwd("HeadSelectViT.norm", dYn, sv["Xlast"].data_ptr(), T * DIM, sv["mun"], sv["rsn"], B, DIM,
                    dX.data_ptr(), T * DIM, 0.0)
        dX = self.headselect_bwd(dX)
        dX = self.encoder_bwd(dX, self.enc, hidden=m.mlp_dim, **ENCODER)
        # embedding
        dXe = self.drop_bwd("emb", dX, B * T * DIM, self.pe)
        dph, dpl = self.new(B * 16, 64), self.new(B * 16, 64)
        part = self.new(B, EMBED_PART)
        L.vc_mhst_embed_bwd(B, sv["ph"].data_ptr(), sv["pl"].data_ptr(), P["weight_hsi"], P["weight_lidar"],
                            P["encoder_embedding.weight"], dXe.data_ptr(), dxcnn.data_ptr(), dph.data_ptr(),
                            dpl.data_ptr(), part.data_ptr(), s)
        self.reduce_part(part, EMBED_PART, 0, 1024, G["encoder_embedding.weight"])
        self.reduce_part(part, EMBED_PART, 1024, 64, G["encoder_embedding.bias"])
        self.reduce_part(part, EMBED_PART, 1088, 64, G["encoder_pos_embed"])
        self.reduce_part(part, EMBED_PART, 1152, 1, G["weight_hsi"])
        self.reduce_part(part, EMBED_PART, 1153, 1, G["weight_lidar"])
        scr, ns = self.scr.data_ptr(), self.SCRATCH
        L.vc_colsum(B, 64 * DIM, dXe.data_ptr() + F32 * DIM, T * DIM, G["encoder_pos_embed"] + F32 * DIM, 0.0, scr, ns, s)
        L.vc_colsum(B, DIM, dXe.data_ptr(), T * DIM, G["cls_token"], 0.0, scr, ns, s)
        # LiDAR encoder (x2 is data: no input gradient)
        dzl3 = self.new(M2, 64)
        L.vc_maxpool2_bwd(B, 8, 8, 64, dpl.data_ptr(), sv["argl"].data_ptr(), dzl3.data_ptr(), 64, s)
        dyl3 = self.bn_bwd("lidar_encoder.bn3", dzl3, sv["yl3"], sv["meanl3"], sv["invl3"], M2, 64)
        dzl2 = self.linear_bwd(dyl3, sv["zl2"], M2, 64, 64, "lidar_encoder.conv3")
        dyl2 = self.bn_bwd("lidar_encoder.bn2", dzl2, sv["yl2"], sv["meanl2"], sv["invl2"], M2, 64)
        dzl1 = self.new(M2, 32)
        for i, shp in enumerate(sh["l2"]):
            self.conv_bwd(shp, sv["zl1"], 32, f"lidar_encoder.conv2.conv2_{i + 1}.weight", None, dyl2, 16 * i, 64, dzl1,
                          1.0 if i else 0.0)
        dyl1 = self.bn_bwd("lidar_encoder.bn1", dzl1, sv["yl1"], sv["meanl1"], sv["invl1"], M2, 32)
        for i, shp in enumerate(sh["l1"]):
            self.conv_bwd(shp, sv["x2r"], sv["ld2"], f"lidar_encoder.conv1.conv2_{i + 1}.weight", None, dyl1, 8 * i, 32)
        # HSI encoder (x1 is data)
        dz5 = self.new(M2, 64)
        L.vc_maxpool2_bwd(B, 8, 8, 64, dph.data_ptr(), sv["argh"].data_ptr(), dz5.data_ptr(), 64, s)
        dy5 = self.bn_bwd("hsi_encoder.bn5", dz5, sv["y5"], sv["mean5"], sv["inv5"], M2, 64)
        dz4 = self.linear_bwd(dy5, sv["z4"], M2, 64, 64, "hsi_encoder.conv5")
        dy4 = self.bn_bwd("hsi_encoder.bn4", dz4, sv["y4"], sv["mean4"], sv["inv4"], M2, 64)
        dz3 = self.new(M3, 16)
        for i, shp in enumerate(sh["h4"]):
            self.conv_bwd(shp, sv["z3"], 16, f"hsi_encoder.conv4.conv2_{i + 1}.weight", None, dy4, 16 * i, 64, dz3,
                          1.0 if i else 0.0)
        dy3 = self.bn_bwd("hsi_encoder.bn3", dz3, sv["y3"], sv["mean3"], sv["inv3"], M3, 16)
        dz2 = self.new(M3, 16)
        L.vc_mhst_conv3_wgrad(B, D1, sv["z2"].data_ptr(), 16, dy3.data_ptr(), 16, G["hsi_encoder.conv3.weight"], scr, ns,
                              s)
        L.vc_colsum(M3, 16, dy3.data_ptr(), 16, G["hsi_encoder.conv3.bias"], 0.0, scr, ns, s)
        L.vc_mhst_conv3_dgrad(B, D1, dy3.data_ptr(), 16, P["hsi_encoder.conv3.weight"], dz2.data_ptr(), 16, 0.0, s)
        dy2 = self.bn_bwd("hsi_encoder.bn2", dz2, sv["y2"], sv["mean2"], sv["inv2"], M3, 16)
        dz1 = self.new(M3, 16)
        spectral = [f"hsi_encoder.conv2_{i + 1}" for i in range(len(SPECTRAL_TAPS))]
        if self.front:
            L.vc_mhst_sconv_wgrad(B, D1, sv["z1"].data_ptr(), 16, dy2.data_ptr(), 16,
                                  *(G[pf + ".weight"] for pf in spectral), *(G[pf + ".bias"] for pf in spectral), scr, ns,
                                  s)
            L.vc_mhst_sconv_dgrad(B, D1, dy2.data_ptr(), 16, *(P[pf + ".weight"] for pf in spectral), dz1.data_ptr(), 16,
                                  0.0, scr, ns, s)
        else:
            for i, (pf, shp) in enumerate(zip(spectral, sh["h2"])):
                self.conv_bwd(shp, sv["z1"], 16, pf + ".weight", pf + ".bias", dy2, 4 * i, 16, dz1, 1.0 if i else 0.0)
        dy1 = self.bn_bwd("hsi_encoder.bn1", dz1, sv["y1"], sv["mean1"], sv["inv1"], M3, 16)
        if self.front:
            L.vc_mhst_conv1_wgrad(B, m.l1, self.x1.data_ptr(), dy1.data_ptr(), 16, G["hsi_encoder.conv1.weight"],
                                  G["hsi_encoder.conv1.bias"], scr, ns, s)
        else:
            self.conv_bwd(sh["h1"], self.x1, 1, "hsi_encoder.conv1.weight", "hsi_encoder.conv1.bias", dy1, 0, 16)
        self.sv, self.enc, self.hs = {}, [], []
        return grad

    def headselect_bwd(self, dX):
        m, L, B, P, s = self.m, self.L, self.B, self.P, self.s
        R, Hh = B * T, m.hs_hidden
        G = self.G
        for i in reversed(range(m.hs_depth)):
            pre = f"HeadSelectViT.blocks.{i}"
            st = self.hs[i]
            sel = st["sel"]
            dsel = self.new(B, HS_HEADS)
            # MLP: X3 = X2 + drop(fc2(drop(gelu(fc1(mask(LN2(X2)))))))
            dF2 = self.drop_bwd(f"hs{i}.fc2", dX, R * DIM, st["pm"])
            dGd = self.linear_bwd(dF2, st["Gd"], R, Hh, DIM, pre + ".mlp.fc2")
            dGl = self.drop_bwd(f"hs{i}.fc1", dGd, R * Hh, st["pm"])
            dH1 = self.new(R, Hh)
            L.vc_gelu_bwd(R * Hh, dGl.data_ptr(), st["H1"].data_ptr(), dH1.data_ptr(), s)
            dym = self.linear_bwd(dH1, st["ym"], R, DIM, Hh, pre + ".mlp.fc1")
            dY2 = self.new(R, DIM)
            L.vc_mhst_headmask_bwd(B, T, DIM, dym.data_ptr(), st["Y2"].data_ptr(), sel.data_ptr(), dY2.data_ptr(),
                                   dsel.data_ptr(), 0.0, s)
            dX2 = self.new(R, DIM)
            L.vc_add2_2d(R, DIM, dX.data_ptr(), DIM, None, 0, dX2.data_ptr(), DIM, 0.0, s)
            self.ln_bwd(pre + ".norm2", dY2, st["X2"].data_ptr(), DIM, st["mu2"], st["rs2"], R, DIM, dX2.data_ptr(), DIM,
                        1.0)
            # attention: X2 = X + drop(proj(mask(attn(pool(mask(qkv(LN1(X))))))))
            dpr = self.drop_bwd(f"hs{i}.proj", dX2, R * DIM, st["pj"])
            dam = self.linear_bwd(dpr, st["am"], R, DIM, DIM, pre + ".attn.proj")
            # the fused chain backwards: dam -> dqkv, the pooling parameters' per-(sample, head) partials and, with the
            # MLP mask's share in dsel, the gate's dlogits (straight-through)
            dqkv, part, dlg = self.new(R, 3 * DIM), self.new(B * HS_HEADS, POOL_FLOATS), self.new(B, HS_HEADS)
            L.vc_mhst_hsattn_bwd(B, st["qkv"].data_ptr(), sel.data_ptr(), st["yg"].data_ptr(),
                                 P[pre + ".attn.pool_q.weight"], LN_EPS, 0.5, st["pp"],
                                 st["mk"].data_ptr() if st["mk"] is not None else None, dam.data_ptr(), dsel.data_ptr(),
                                 1.0 / m.head_tau if self.train else 1.0, dqkv.data_ptr(), part.data_ptr(),
                                 dlg.data_ptr(), s)
            L.vc_colsum(B * HS_HEADS, POOL_FLOATS, part.data_ptr(), POOL_FLOATS, G[pre + ".attn.pool_q.weight"], 0.0,
                        self.scr.data_ptr(), self.SCRATCH, s)
            self.gemm(1, 0, 3 * DIM, DIM, R, dqkv.data_ptr(), 3 * DIM, st["Y"].data_ptr(), DIM,
                      G[pre + ".attn.query.weight"], DIM)
            dY = self.new(R, DIM)
            self.gemm(0, 0, R, DIM, 3 * DIM, dqkv.data_ptr(), 3 * DIM, P[pre + ".attn.query.weight"], DIM, dY.data_ptr(),
                      DIM)
            dXi = self.new(R, DIM)
            L.vc_add2_2d(R, DIM, dX2.data_ptr(), DIM, None, 0, dXi.data_ptr(), DIM, 0.0, s)
            self.ln_bwd(pre + ".norm1", dY, st["X"].data_ptr(), DIM, st["mu"], st["rs"], R, DIM, dXi.data_ptr(), DIM,
                        1.0)
            # the gate's Linear on the cls rows (ld T * DIM)
            gp = pre + ".head_select.mlp_head"
            self.gemm(1, 0, HS_HEADS, DIM, B, dlg.data_ptr(), HS_HEADS, st["X"].data_ptr(), T * DIM, G[gp + ".weight"], DIM,
                      bias_grad=G[gp + ".bias"])
            self.gemm(0, 0, B, DIM, HS_HEADS, dlg.data_ptr(), HS_HEADS, P[gp + ".weight"], DIM, dXi.data_ptr(), T * DIM,
                      beta=1.0)
            dX = dXi
        return dX
