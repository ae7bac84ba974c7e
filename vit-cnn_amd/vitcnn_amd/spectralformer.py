"""SpectralFormer comparison model (per-pixel band transformer) on the MI355X path.

Reference: `model/compare_method/spectralformer.py` (class `SpectralFormer` :111-156, `Transformer` :77-109), built by
`model_utils.py:377-399` (image_size = patch_size = 1, near_band 1, num_patches = n_bands + n_bands2, dim 64, depth 5,
heads 4, mlp_dim 8, dropout 0.1, emb_dropout 0.1, mode 'ViT', Adam lr 5e-4 = the fused `AdamW(weight_decay=0)`).

The module keeps the reference's parameter tree (69 `state_dict` keys, creation order and initialisers, so the same
`torch.manual_seed` draws the same values), including the three `transformer.skipcat.*` convolutions 'ViT' mode never
applies: they live in the flat buffer, get a zero gradient and stay bit-unchanged under the fused optimizer.

Every band of the pixel's concatenated spectrum is one token: `patch_to_embedding` is `Linear(1, dim)`, an outer
product, so the token rows come from one kernel (`vc_sf_embed_fwd`: cls row, x w + bias, position, embedding dropout)
instead of a GEMM.  Everything behind the embedding -- five pre-norm layers, the head on the cls row, the four dropout
sites, the grouped weight-gradient GEMMs -- is S2EFT's program (`s2eft._Program.layers` / `layers_bwd`) in 'ViT' mode.
Dropout uses `vc_dropout_fwd`'s counter hash with S2EFT's seeding (torch's CPU generator, the rank mixed in).

Deviations: the constructor accepts what the reference's forward can run (image_size 1, near_band 1, mode 'ViT') within
the attention kernel's envelope (dim_head 16, num_patches + 1 <= 256 tokens) and raises ValueError otherwise; `mask`
raises NotImplementedError (the reference's mask path needs an un-imported name, as S2EFT's).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import program, s2eft
from .flat import FlatParams

T_MAX = 256   # vc_s2eft_attn_*'s bound on the token count


class SpectralFormer(FlatParams, nn.Module):
    """Same constructor as the reference class; forward(x1 [B, C1] or [B, C1, 1, 1], x2 likewise) -> logits."""

    def __init__(self, image_size, near_band, num_patches, num_classes, dim, depth, heads, mlp_dim, pool="cls",
                 channels=1, dim_head=16, dropout=0.0, emb_dropout=0.0, mode="ViT"):
        super().__init__()
        if image_size != 1 or near_band != 1:
            raise ValueError("SpectralFormer MI355X path: per-pixel tokens only (image_size 1, near_band 1): the "
                             f"reference's forward feeds Linear(1, dim); got {image_size}, {near_band}")
        if mode != "ViT":
            raise ValueError(f"SpectralFormer MI355X path: mode 'ViT' only, got {mode!r}")
        if dim_head != 16:
            raise ValueError("SpectralFormer MI355X path: the attention kernel is written for dim_head 16")
        if not 2 <= num_patches + 1 <= T_MAX:
            raise ValueError(f"SpectralFormer MI355X path: num_patches + 1 must be in 2..{T_MAX}, got {num_patches + 1}")
        if depth < 1 or heads < 1 or dim < 1 or mlp_dim < 1 or num_classes < 2:
            raise ValueError("SpectralFormer MI355X path: depth, heads, dim, mlp_dim >= 1 and num_classes >= 2")
        patch_dim = image_size ** 2 * near_band
        # creation order = the reference's (:117-130), so the default initialisation draws the same numbers
        self.pos_embedding = nn.Parameter(torch.randn(1, num_patches + 1, dim))
        self.patch_to_embedding = nn.Linear(patch_dim, dim)
        self.cls_token = nn.Parameter(torch.randn(1, 1, dim))
        self.dropout = nn.Dropout(emb_dropout)
        self.transformer = s2eft.Transformer(dim, depth, heads, dim_head, mlp_dim, dropout, num_patches, mode)
        self.pool = pool
        self.to_latent = nn.Identity()
        self.mlp_head = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, num_classes))
        # the attributes s2eft._Program reads: N tokens in front of the cls row, T = N + 1
        self.N, self.C, self.D, self.depth, self.heads = num_patches, patch_dim, dim, depth, heads
        self.hidden, self.ncls, self.mode = mlp_dim, num_classes, mode
        self.p_drop, self.p_emb = float(dropout), float(emb_dropout)
        self._build_flat()

    def forward(self, x1: torch.Tensor, x2: torch.Tensor, mask=None) -> torch.Tensor:
        if mask is not None:
            raise NotImplementedError("SpectralFormer mask path is not supported (the reference's raises, :62)")
        if x1.device.type != "cuda" or x2.device.type != "cuda":
            raise RuntimeError("SpectralFormer MI355X path: inputs must be on a ROCm (cuda) device; no CPU fallback")
        x1, x2 = _pixel_rows(x1, "x1"), _pixel_rows(x2, "x2")
        if x1.shape[0] != x2.shape[0] or x1.shape[1] + x2.shape[1] != self.N:
            raise RuntimeError(f"expected x1 [B, C1] and x2 [B, C2] with C1 + C2 = {self.N}, got {list(x1.shape)} / "
                               f"{list(x2.shape)}")
        return program.run(self, _Program, x1, x2)


def _pixel_rows(x, name):
    """[B, C] or [B, C, 1, 1] (what PatchBatcher / SlidingWindowInference yield at patch_size 1: the same memory) as
    contiguous fp32 rows [B, C]"""
    if x.dim() == 4 and x.shape[2] == 1 and x.shape[3] == 1:
        x = x.reshape(x.shape[0], x.shape[1])
    if x.dim() != 2 or x.shape[1] < 1:
        raise RuntimeError(f"expected {name} [B, C] or [B, C, 1, 1], got {list(x.shape)}")
    return x.detach().to(torch.float32).contiguous()


class _Program(s2eft._Program):
    """S2EFT's program with the per-band embedding in place of the gate + patch GEMM"""

    NAME = "SpectralFormer"

    def __init__(self, m, needs_grad, x1, x2):
        super().__init__(m, needs_grad, x1)
        self.x1, self.x2 = x1, x2
        self.C1, self.C2 = x1.shape[1], x2.shape[1]

    def embed(self):
        B, T, D, P = self.B, self.T, self.m.D, self.P
        X = self.new(B, T, D)
        mk = None
        if self.pe > 0:
            mk = torch.empty(B * T * D, dtype=torch.uint8, device=self.dev)
            self.masks["emb"] = mk    # site 0 of the seed sequence, as s2eft's drop("emb", ...)
        if mk is not None and self.dseed is not None:   # the attached device seed, site offset 0
            self.L.vc_sf_embed_fwd_ds(B, self.C1, self.C2, D, self.x1.data_ptr(), self.x2.data_ptr(),
                                      P["patch_to_embedding.weight"], P["patch_to_embedding.bias"], P["cls_token"],
                                      P["pos_embedding"], self.pe, self.dseed.cur_ptr, 0, X.data_ptr(), mk.data_ptr(),
                                      self.s)
            return X
        self.L.vc_sf_embed_fwd(B, self.C1, self.C2, D, self.x1.data_ptr(), self.x2.data_ptr(),
                               P["patch_to_embedding.weight"], P["patch_to_embedding.bias"], P["cls_token"],
                               P["pos_embedding"], self.pe, self.seed % (1 << 63), X.data_ptr(),
                               mk.data_ptr() if mk is not None else None, self.s)
        return X

    def embed_bwd(self, dX, G, sd, side):
        from functools import partial
        mk = self.masks["emb"] if self.pe > 0 else None
        side((dX,), partial(self.L.vc_sf_embed_bwd, self.B, self.C1, self.C2, self.m.D, self.x1.data_ptr(),
                            self.x2.data_ptr(), dX.data_ptr(), mk.data_ptr() if mk is not None else None, self.pe,
                            G["patch_to_embedding.weight"], G["patch_to_embedding.bias"], G["pos_embedding"],
                            G["cls_token"], sd[1], self.SCRATCH, sd[0]))
