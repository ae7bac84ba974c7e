"""Plugin surface of the reference (`model_utils.py`) for the ViT-CNN path, over the MI355X model.

Same names, arguments, defaults and error behaviour as the reference functions this file
replaces, so `main.py`-style drivers switch by changing one import:

* `get_model(name, **kwargs) -> (model, optimizer, criterion, kwargs)`  — model_utils.py:47-511,
  ViT-CNN branch :297-313, defaults :493-510, unknown name -> KeyError (:488-489).
* `train(savename, run, bands, net, optimizer, criterion, data_loader, epoch, ...)` — :854-1045.
* `save_model(savename, model, model_name, dataset_name, train_state, type, **kwargs)` — :1047-1064.
* `test(run, net, img1, img2, hyperparams) -> probs[W, H, n_classes]` — :1067-1132.
* `val(net, data_loader, device, supervision) -> accuracy` — :1135-1158.
* `predict(run, net, img1, img2, hyperparams, centers=None) -> labels[W, H]` (device, int64) and
  `evaluate(run, net, img1, img2, gt, hyperparams) -> metrics dict` — main.py:500-519 (test, argmax, metrics) on the
  device, over the labelled pixels only; `hyperparams["border"]` mirrors the scene's edges.

Registered: "Multimodality_Mamba" (the README's "ViT-CNN (ours)"), "S2EFT" (config 5, :400-423),
"FusAtNet" (config 5, :109-118), "MFT" (:364-376) and the four MDL-RS baselines "Early_fusion_CNN",
"Middle_fusion_CNN", "Late_fusion_CNN" and "Cross_fusion_CNN" (:69-108; the last trains with
`Cross_fusion_CNN_Loss` over its three outputs, and `val` / `test` read the first), and the per-pixel models
"EndNet" (:119-128, `EndNet_Loss` over its five outputs) and "SpectralFormer" (:377-399), both with patch_size 1, and
"HCTnet" (:351-363; the HSI cube reduced to 3 principal components, `PatchBatcher(applyPCA=True)`) and "MHST"
(:314-335; patch_size 8), and "GLT_Net" (no branch in the reference's registry: this project's defaults, `_get_glt`;
patch_size 24 = three times the model's 8, the three scales being centre crops of one window; `GLT_Loss`).
The reference's other branches import modules absent from the reference tree (SURVEY.md section 2a
row 22) and are out of scope for this path.

Data parallelism: when a torch.distributed process group with more than
one rank is initialised, `train` starts every replica from rank 0's parameters, all-reduces the
gradient after every backward (RCCL) and folds the 1/world average into the fused AdamW update;
each rank iterates its own shard of the batches (a loader that is not already sharded is wrapped in
`parallel.ShardedLoader`, which shards a torch DataLoader at its sampler).

Precision (BASELINE.json config 2): `get_model(..., precision="bf16")` builds ViT-CNN with bf16
GEMM operands and fp32 accumulation (`Multimodality_Mamba.set_precision`), and FusAtNet with bf16 operands on
its 3x3 convolutions (`FusAtNet.set_precision`; FusAtNet alone also takes "bf16_store", the same
contract over operands kept as bf16 in memory, section 30); the default "fp32" is the parity mode.
The other models have no bf16 mode.
"""
from __future__ import annotations

import copy
import datetime
import os
import re

import numpy as np
import torch

from . import parallel
from .losses import CrossEntropyLoss
from .model import Multimodality_Mamba
from .optim import AdamW
from .window import SlidingWindowInference

MDLRS = ("Early_fusion_CNN", "Middle_fusion_CNN", "Late_fusion_CNN", "Cross_fusion_CNN")
REGISTERED = ("Multimodality_Mamba", "S2EFT", "FusAtNet", "MFT") + MDLRS + ("EndNet", "SpectralFormer", "HCTnet", "MHST", "GLT_Net")


def camel_to_snake(name: str) -> str:
    """utils.py camel_to_snake: 'Multimodality_Mamba' -> 'multimodality__mamba'."""
    s = re.sub("(.)([A-Z][a-z]+)", r"\1_\2", name)
    return re.sub("([a-z0-9])([A-Z])", r"\1_\2", s).lower()


def get_model(name, **kwargs):
    """Instantiate the model, optimizer and criterion with the reference's defaults.

    Required kwargs (as in the reference): n_classes, n_bands=(hsi_bands, lidar_bands),
    ignored_labels, dataset.  `device` defaults to the first ROCm device (the MI355X path has no
    CPU execution; the reference defaults to CPU).
    """
    if name not in REGISTERED:
        raise KeyError("{} model is unknown.".format(name))
    device = kwargs.setdefault("device", torch.device("cuda" if torch.cuda.is_available() else "cpu"))
    n_classes = kwargs["n_classes"]
    (n_bands, n_bands2) = kwargs["n_bands"]
    weights = torch.ones(n_classes)
    weights[torch.LongTensor(list(kwargs["ignored_labels"]))] = 0.0
    weights = weights.to(device)
    weights = kwargs.setdefault("weights", weights)
    if name == "S2EFT":
        return _get_s2eft(n_bands, n_classes, device, kwargs)
    if name == "FusAtNet":
        return _get_fusatnet(n_bands, n_bands2, n_classes, device, kwargs)
    if name == "MFT":
        return _get_mft(n_bands, n_bands2, n_classes, device, kwargs)
    if name in MDLRS:
        return _get_mdlrs(name, n_bands, n_bands2, n_classes, device, kwargs)
    if name == "EndNet":
        return _get_endnet(n_bands, n_bands2, n_classes, device, kwargs)
    if name == "SpectralFormer":
        return _get_spectralformer(n_bands, n_bands2, n_classes, device, kwargs)
    if name == "HCTnet":
        return _get_hctnet(n_bands, n_classes, device, kwargs)
    if name == "MHST":
        return _get_mhst(n_bands, n_bands2, n_classes, device, kwargs)
    if name == "GLT_Net":
        return _get_glt(n_bands, n_bands2, n_classes, device, kwargs)
    kwargs.setdefault("patch_size", 9)
    patch_size = kwargs["patch_size"]
    center_pixel = True
    embed_dim = 64 // 2
    kwargs.setdefault("applyPCA", False)
    if kwargs["applyPCA"]:
        n_bands = 30
        kwargs.setdefault("pca_components", 30)   # what PatchBatcher / test() must reduce the cube to (pca.py)
    path_type = "multi_clock_gate"
    precision = kwargs.setdefault("precision", "fp32")
    model = Multimodality_Mamba(img_size=patch_size, patch_size=1, stride=1, in_channels1=n_bands,
                                in_channels2=n_bands2, dim_embedding=embed_dim, num_class=n_classes,
                                path_type=path_type, precision=precision)
    lr = kwargs.setdefault("lr", 8e-4)
    model = model.to(device)
    optimizer = AdamW(model.parameters(), lr=lr)
    criterion = CrossEntropyLoss(weight=kwargs["weights"])
    kwargs.setdefault("epoch", 200)
    kwargs.setdefault("batch_size", 64)
    kwargs.setdefault("scheduler", torch.optim.lr_scheduler.StepLR(optimizer, step_size=30, gamma=0.9))
    kwargs.setdefault("supervision", "full")
    kwargs.setdefault("flip_augmentation", False)
    kwargs.setdefault("radiation_augmentation", False)
    kwargs.setdefault("mixture_augmentation", False)
    kwargs["center_pixel"] = center_pixel
    return model, optimizer, criterion, kwargs


def _get_s2eft(n_bands, n_classes, device, kwargs):
    """S2EFT branch of model_utils.py:400-423 (config 5): ViT(image_size=patch_size, near_band 3,
    num_patches=n_bands, dim 64, depth 5, heads 4, mlp_dim 8, dropout 0.1, mode 'CAF'), Adam(lr 5e-4),
    weighted CE, epoch 600, batch 64.  Adam = the fused AdamW kernel with weight_decay 0.  The model is
    `s2eft.S2EFT`, the reference's `ViT` over the two patches: forward(x1 [B, n_bands, P, P], x2 [B, 1, P, P]) forms
    the neighbour-band token rows [B, n_bands + 1, patch_size**2 * 3] on the device (SURVEY.md section 8 row A13,
    DESIGN.md section 26), so `train` / `val` / `test` run it like every other model (one LiDAR band, as the
    reference's num_patches = n_bands implies)."""
    from .s2eft import S2EFT
    kwargs.setdefault("patch_size", 7)
    kwargs.setdefault("applyPCA", False)
    if kwargs["applyPCA"]:
        n_bands = 30
        kwargs.setdefault("pca_components", 30)   # what PatchBatcher / test() must reduce the cube to (pca.py)
    model = S2EFT(image_size=kwargs["patch_size"], near_band=3, num_patches=n_bands, num_classes=n_classes, dim=64,
                  depth=5, heads=4, mlp_dim=8, dropout=0.1, emb_dropout=0.1, mode="CAF").to(device)
    lr = kwargs.setdefault("lr", 0.0005)
    optimizer = AdamW(model.parameters(), lr=lr, weight_decay=0.0)
    criterion = CrossEntropyLoss(weight=kwargs["weights"])
    kwargs.setdefault("epoch", 600)
    kwargs.setdefault("batch_size", 64)
    kwargs.setdefault("supervision", "full")
    kwargs["center_pixel"] = True
    return model, optimizer, criterion, kwargs


def _get_fusatnet(n_bands, n_bands2, n_classes, device, kwargs):
    """FusAtNet branch of model_utils.py:109-118: FusAtNet(n_bands, n_bands2, n_classes), patch 11,
    Adam(lr 1e-3) as in the reference -- the fused AdamW kernel with weight_decay 0 over the model's flat
    parameter buffer (torch.optim.Adam's update exactly) --, weighted CE, epoch 150, batch 64, applyPCA False.
    The reference's backward raises (in-place residual add); this path trains with
    out-of-place residual semantics (vitcnn_amd/fusatnet.py).  `precision="bf16"`: bf16 operands on the 3x3 convs
    (`FusAtNet.set_precision`); `precision="bf16_store"`: those operands stored as bf16
    (section 30)."""
    from .fusatnet import FusAtNet
    kwargs.setdefault("patch_size", 11)
    precision = kwargs.setdefault("precision", "fp32")
    model = FusAtNet(n_bands, n_bands2, n_classes, precision=precision).to(device)
    lr = kwargs.setdefault("lr", 0.001)
    optimizer = AdamW(model.parameters(), lr=lr, weight_decay=0.0)
    criterion = CrossEntropyLoss(weight=kwargs["weights"])
    kwargs.setdefault("epoch", 150)
    kwargs.setdefault("batch_size", 64)
    kwargs.setdefault("applyPCA", False)
    kwargs.setdefault("supervision", "full")
    kwargs["center_pixel"] = True
    return model, optimizer, criterion, kwargs


def _get_mft(n_bands, n_bands2, n_classes, device, kwargs):
    """MFT branch of model_utils.py:364-376: MFT(patch_size, FM 16, NC n_bands (30 under applyPCA), NCLidar n_bands2,
    HSIOnly False), patch 11, Adam(lr 5e-4, weight_decay 5e-3) -- torch.optim.Adam's coupled L2 decay, the fused
    `vitcnn_amd.optim.Adam` over the flat buffer --, weighted CE, epoch 500, batch 64."""
    from .mft import MFT
    from .optim import Adam
    kwargs.setdefault("patch_size", 11)
    kwargs.setdefault("applyPCA", False)
    if kwargs["applyPCA"]:
        n_bands = 30
        kwargs.setdefault("pca_components", 30)   # what PatchBatcher / test() must reduce the cube to (pca.py)
    model = MFT(patch_size=kwargs["patch_size"], FM=16, NC=n_bands, NCLidar=n_bands2, Classes=n_classes,
                HSIOnly=False).to(device)
    lr = kwargs.setdefault("lr", 0.0005)
    optimizer = Adam(model.parameters(), lr=lr, weight_decay=5e-3)
    criterion = CrossEntropyLoss(weight=kwargs["weights"])
    kwargs.setdefault("epoch", 500)
    kwargs.setdefault("batch_size", 64)
    kwargs.setdefault("supervision", "full")
    kwargs["center_pixel"] = True
    return model, optimizer, criterion, kwargs


def _get_mdlrs(name, n_bands, n_bands2, n_classes, device, kwargs):
    """The four MDL-RS branches of model_utils.py:69-108, which differ in the class and the criterion only:
    <name>(n_bands, n_bands2, n_classes), patch 7, Adam(lr 1e-3) -- the fused AdamW kernel with weight_decay 0, as
    FusAtNet --, weighted CE (Cross_fusion_CNN: Cross_fusion_CNN_Loss(weight)), epoch 150, batch 64, applyPCA False
    (it does not change n_bands here, as in the reference)."""
    from . import mdlrs
    from .losses import Cross_fusion_CNN_Loss
    kwargs.setdefault("patch_size", 7)
    model = getattr(mdlrs, name)(n_bands, n_bands2, n_classes, patch_size=kwargs["patch_size"]).to(device)
    lr = kwargs.setdefault("lr", 0.001)
    optimizer = AdamW(model.parameters(), lr=lr, weight_decay=0.0)
    if name == "Cross_fusion_CNN":
        criterion = Cross_fusion_CNN_Loss(weight=kwargs["weights"])
    else:
        criterion = CrossEntropyLoss(weight=kwargs["weights"])
    kwargs.setdefault("epoch", 150)
    kwargs.setdefault("batch_size", 64)
    kwargs.setdefault("applyPCA", False)
    kwargs.setdefault("supervision", "full")
    kwargs["center_pixel"] = True
    return model, optimizer, criterion, kwargs


def _get_endnet(n_bands, n_bands2, n_classes, device, kwargs):
    """EndNet branch of model_utils.py:119-128: EndNet(n_bands, n_bands2, n_classes), patch 1 (a pixel's two spectra),
    Adam(lr 1e-3) -- the fused AdamW kernel with weight_decay 0, as FusAtNet --, EndNet_Loss(weight), epoch 150, batch 64,
    applyPCA False (it does not change n_bands here, as in the reference)."""
    from .endnet import EndNet
    from .losses import EndNet_Loss
    kwargs.setdefault("patch_size", 1)
    model = EndNet(n_bands, n_bands2, n_classes).to(device)
    lr = kwargs.setdefault("lr", 0.001)
    optimizer = AdamW(model.parameters(), lr=lr, weight_decay=0.0)
    criterion = EndNet_Loss(weight=kwargs["weights"])
    kwargs.setdefault("epoch", 150)
    kwargs.setdefault("batch_size", 64)
    kwargs.setdefault("applyPCA", False)
    kwargs.setdefault("supervision", "full")
    kwargs["center_pixel"] = True
    return model, optimizer, criterion, kwargs


def _get_spectralformer(n_bands, n_bands2, n_classes, device, kwargs):
    """SpectralFormer branch of model_utils.py:377-399: SpectralFormer(image_size=patch_size, near_band 1, num_patches =
    n_bands + n_bands2 (n_bands 30 under applyPCA), dim 64, depth 5, heads 4, mlp_dim 8, dropout 0.1, emb_dropout 0.1,
    mode 'ViT'), patch 1, Adam(lr 5e-4) as the fused AdamW with weight_decay 0, weighted CE, epoch 300, batch 64."""
    from .spectralformer import SpectralFormer
    kwargs.setdefault("patch_size", 1)
    kwargs.setdefault("applyPCA", False)
    if kwargs["applyPCA"]:
        n_bands = 30
        kwargs.setdefault("pca_components", 30)   # what PatchBatcher / test() must reduce the cube to (pca.py)
    model = SpectralFormer(image_size=kwargs["patch_size"], near_band=1, num_patches=n_bands + n_bands2,
                           num_classes=n_classes, dim=64, depth=5, heads=4, mlp_dim=8, dropout=0.1, emb_dropout=0.1,
                           mode="ViT").to(device)
    lr = kwargs.setdefault("lr", 0.0005)
    optimizer = AdamW(model.parameters(), lr=lr, weight_decay=0.0)
    criterion = CrossEntropyLoss(weight=kwargs["weights"])
    kwargs.setdefault("epoch", 300)
    kwargs.setdefault("batch_size", 64)
    kwargs.setdefault("supervision", "full")
    kwargs["center_pixel"] = True
    return model, optimizer, criterion, kwargs


def _get_hctnet(n_bands, n_classes, device, kwargs):
    """HCTnet branch of model_utils.py:351-363: HCTnet(num_classes, num_tokens 6, heads 8) -- no band count is passed:
    the model takes the HSI cube reduced to 3 components, which `applyPCA` (default True here) makes of it in
    `PatchBatcher(applyPCA=True)` and `test()` --, patch 11, Adam(lr 1e-4) as the fused AdamW with weight_decay 0,
    weighted CE, epoch 100, batch 64.  n_bands = 30 under applyPCA is the reference's line and is unused."""
    from .hctnet import HCTnet
    kwargs.setdefault("patch_size", 11)
    kwargs.setdefault("applyPCA", True)
    if kwargs["applyPCA"]:
        n_bands = 30   # noqa: F841 (as the reference writes it; the constructor takes no band count)
        kwargs.setdefault("pca_components", 3)   # the model's HSI depth (hctnet.py)
    model = HCTnet(num_classes=n_classes, num_tokens=6, heads=8).to(device)
    lr = kwargs.setdefault("lr", 0.0001)
    optimizer = AdamW(model.parameters(), lr=lr, weight_decay=0.0)
    criterion = CrossEntropyLoss(weight=kwargs["weights"])
    kwargs.setdefault("epoch", 100)
    kwargs.setdefault("batch_size", 64)
    kwargs.setdefault("supervision", "full")
    kwargs["center_pixel"] = True
    return model, optimizer, criterion, kwargs


def _get_mhst(n_bands, n_bands2, n_classes, device, kwargs):
    """MHST branch of model_utils.py:314-335: MHST(l1, l2, patch 8, width 64, en_depth 5 of 4 heads, mlp_dim 8, dropout
    0.1, coefficient_hsi 0.6, coefficient_vit 0.7, 8 head-select blocks of 16 heads, tau 5, no qkv bias, mlp_ratio 4),
    AdamW(lr 8e-4), weighted CE over the model's mixture of probabilities, epoch 1000, batch 64; under applyPCA the
    model is built for 30 bands.  `conv="mfma"`: the pyramidal convolutions on the fp32 MFMA (`MHST.set_conv`, DESIGN.md
    section 28); `conv="mfma_all"`: those plus `hsi_encoder.conv1` and the four spectral convolutions (as one) on the
    MFMA; the default "direct" is the recorded program."""
    from .mhst import MHST
    kwargs.setdefault("patch_size", 8)
    conv = kwargs.setdefault("conv", "direct")
    kwargs.setdefault("applyPCA", False)
    if kwargs["applyPCA"]:
        n_bands = 30
        kwargs.setdefault("pca_components", 30)   # what PatchBatcher / test() must reduce the cube to (pca.py)
    model = MHST(l1=n_bands, l2=n_bands2, patch_size=kwargs["patch_size"], num_patches=64, num_classes=n_classes,
                 encoder_embed_dim=64, en_depth=5, en_heads=4, mlp_dim=8, dropout=0.1, emb_dropout=0.1,
                 coefficient_hsi=0.6, coefficient_vit=0.7, hsp_vit_depth=8, hsp_vit_num_heads=16, head_tau=5,
                 use_head_select=True, vit_qkv_bias=False, mlp_ratio=4, attnproj_mlp_drop=0.1, attn_drop=0.1,
                 conv=conv).to(device)
    lr = kwargs.setdefault("lr", 8e-4)
    optimizer = AdamW(model.parameters(), lr=lr)
    criterion = CrossEntropyLoss(weight=kwargs["weights"])
    kwargs.setdefault("epoch", 1000)
    kwargs.setdefault("batch_size", 64)
    kwargs.setdefault("supervision", "full")
    kwargs["center_pixel"] = True
    return model, optimizer, criterion, kwargs


def _get_glt(n_bands, n_bands2, n_classes, device, kwargs):
    """GLT-Net.  The reference's `get_model` has no branch for this model (its main.py lists it as unusable "for now"),
    so these defaults are THIS PROJECT'S choice, taken from the shapes in the reference module's comments and from the
    sibling transformers' branches: GLT(l1, l2, patch_size 8, num_patches 64, width 64 / decoder width 32, 5 + 5 layers
    of 4 heads of 16, mlp_dim 8, dropout 0.1), Adam(lr 5e-4) as the fused AdamW with weight_decay 0, `GLT_Loss` (weighted
    CE + the model's reconstruction loss), epoch 500, batch 64; under applyPCA the model is built for 30 bands.
    kwargs["patch_size"] is what the batcher and `test()` cut: 24 = 3 * the model's patch side 8
    (kwargs["glt_patch_size"]); a caller who passes patch_size passes the cut size, a multiple of 6."""
    from .glt import GLT
    from .losses import GLT_Loss
    cut = kwargs.setdefault("patch_size", 24)
    if cut % 6 or cut < 6:
        raise ValueError(f"GLT_Net: patch_size is the 3P window the batcher cuts and must be a multiple of 6, got {cut}")
    p = kwargs.setdefault("glt_patch_size", cut // 3)
    if 3 * p != cut:
        raise ValueError(f"GLT_Net: glt_patch_size {p} is not patch_size {cut} / 3")
    kwargs.setdefault("applyPCA", False)
    if kwargs["applyPCA"]:
        n_bands = 30
        kwargs.setdefault("pca_components", 30)   # what PatchBatcher / test() must reduce the cube to (pca.py)
    model = GLT(l1=n_bands, l2=n_bands2, patch_size=p, num_patches=p * p, num_classes=n_classes, encoder_embed_dim=64,
                decoder_embed_dim=32, en_depth=5, en_heads=4, de_depth=5, de_heads=4, mlp_dim=8, dim_head=16, dropout=0.1,
                emb_dropout=0.1).to(device)
    lr = kwargs.setdefault("lr", 0.0005)
    optimizer = AdamW(model.parameters(), lr=lr, weight_decay=0.0)
    criterion = GLT_Loss(weight=kwargs["weights"])
    kwargs.setdefault("epoch", 500)
    kwargs.setdefault("batch_size", 64)
    kwargs.setdefault("supervision", "full")
    kwargs["center_pixel"] = True
    return model, optimizer, criterion, kwargs


def save_model(savename, model, model_name, dataset_name, train_state, type, **kwargs):
    """Checkpoint scheme of model_utils.py:1047-1064: a plain state_dict (the reference's 1704 keys)
    at ./checkpoints/<model>/<dataset>/<train_state>/<type>/<time><savename>_run{run}_epoch{epoch}_{metric:.2f}.pth.
    Only rank 0 writes under data parallelism."""
    if parallel.rank() != 0:
        return None
    model_dir = "./checkpoints/" + model_name + "/" + dataset_name + "/" + train_state + "/" + type + "/"
    time_str = datetime.datetime.now().strftime("%Y_%m_%d_%H_%M_%S")
    os.makedirs(model_dir, exist_ok=True)
    if not isinstance(model, torch.nn.Module):
        raise TypeError("save_model: only torch modules are checkpointed on this path")
    filename = time_str + savename + "_run{run}_epoch{epoch}_{metric:.2f}".format(**kwargs)
    path = model_dir + filename + ".pth"
    if hasattr(model, "snapshot_state_dict"):
        # the flat buffers in one device-to-host copy each (not 1704 per-tensor transfers)
        sd = model.snapshot_state_dict(device="cpu")
    else:
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    torch.save(sd, path)
    return path


def _stepper(net, optimizer, criterion, capture_step=False):
    """the model's TrainStepper for this optimizer / criterion (kept across train() calls, so the
    captured per-shape graphs are reused)"""
    from .step import TrainStepper
    st = getattr(net, "_vc_stepper", None)
    if st is None or st.opt is not optimizer or st.crit is not criterion or \
            st.capture_step != bool(capture_step) or \
            (st.exchange is None) == parallel.is_distributed():
        st = TrainStepper(net, optimizer, criterion, capture_step=capture_step)
        object.__setattr__(net, "_vc_stepper", st)
    return st


def train(savename, run, bands, net, optimizer, criterion, data_loader, epoch, scheduler=None, display_iter=100,
          device=torch.device("cpu"), display=None, val_loader=None, supervision="full", capture_step=False):
    """Training loop of model_utils.py:854-1045: per batch one optimizer step (zero_grad, forward,
    criterion, backward, step: :916-934), the loss recorded per iteration (:936-938) and its running
    mean printed every `display_iter` iterations (:940-962), the scheduler stepped per epoch
    (:997-1000), best-state tracking with best / final checkpoints (:1015-1043).  `display` (visdom)
    is optional here.

    The step is `vitcnn_amd.step.TrainStepper.step`: for ViT-CNN with the fused AdamW one hipGraph
    replay per batch (captured per batch shape; data parallel: bucketed RCCL all-reduce inside it);
    with `capture_step=True` also for the comparison models (MFT, HCTnet, MDL-RS, EndNet, SpectralFormer, S2EFT,
    FusAtNet with the fused optimizer and the package's losses; the dropout masks' seed then lives in device memory
    and every replay draws fresh masks: seeds.py).  `last_stats["launch"]` names the path.
    The per-iteration losses stay on the device and are read in one transfer at each display point
    and at the epoch end (the reference's `loss.item()` host sync per iteration would stall the queue
    every step); the recorded values are the same.

    Data parallel (a process group with more than one rank): replicas start from rank 0's parameters,
    a loader that is not already sharded is wrapped in `parallel.ShardedLoader` (every rank the same
    number of batches: one gradient exchange per batch on every rank; a torch DataLoader is sharded at
    its sampler, so each rank assembles only its own batches), a loader that shards itself
    (PatchBatcher(rank=, world=)) is checked against the group, and the per-epoch metric that
    decides the best-state branch -- whose buffer broadcast is a collective -- is the mean over the
    ranks (validation: accuracy over the union of the ranks' validation batches), so every rank takes
    the same branch.  `train.last_stats` holds per-epoch wall times and batch counts."""
    import time
    if criterion is None:
        raise Exception("Missing criterion. You must specify a loss function.")
    if supervision != "full":
        raise ValueError('supervision mode "{}" is unknown.'.format(supervision))
    net.to(device)
    distributed = parallel.is_distributed()
    if distributed:
        parallel.broadcast_parameters(net)       # replicas start identical (rank 0's values)
        parallel.check_loader_shard(data_loader)  # a self-sharding loader (PatchBatcher) agrees with the group
        if not parallel.is_sharded(data_loader):
            data_loader = parallel.ShardedLoader(data_loader, parallel.rank(), parallel.world())
    stepper = _stepper(net, optimizer, criterion, capture_step)
    save_epoch = 16 if epoch == 128 else (epoch // 20 if epoch > 20 else 1)
    best_val_acc = 0.0
    best_model_wts = None
    losses = []
    iter_ = 1
    val_accuracies = []
    stats = {"epochs": [], "launch": None}
    train.last_stats = stats
    for e in range(1, epoch + 1):
        t_epoch = time.perf_counter()
        net.train()
        pending = []          # device losses not yet read back
        nb = npatch = 0
        avg_loss = 0.0
        n_batches = len(data_loader)
        for batch_idx, (data, data2, target) in enumerate(data_loader):
            loss = stepper.step(data, data2, target)
            if stepper.replays:
                loss = loss.clone()   # a replayed graph's loss buffer is overwritten by the next replay
            pending.append(loss.detach())
            nb += 1
            npatch += int(target.shape[0])
            if display_iter and iter_ % display_iter == 0:
                vals = torch.stack(pending).tolist() if pending else []
                pending = []
                losses.extend(vals)
                if parallel.rank() == 0:
                    mean_loss = float(np.mean(losses[max(0, len(losses) - 101):]))
                    print("Train (epoch {}/{}) [{}/{} ({:.0f}%)]\tLoss: {:.6f}".format(
                        e, epoch, batch_idx * len(data), len(data) * n_batches,
                        100.0 * batch_idx / max(n_batches, 1), mean_loss), flush=True)
                    if display is not None and hasattr(display, "line"):
                        display.line(X=np.arange(len(losses)), Y=np.asarray(losses), win="loss")
            iter_ += 1
        if pending:
            losses.extend(torch.stack(pending).tolist())
        avg_loss = float(np.sum(losses[len(losses) - nb:])) / max(nb, 1) if nb else 0.0
        if val_loader is not None:
            correct, total = _val_counts(net, val_loader, device)
            if distributed:
                correct, total = parallel.sum_over_ranks([correct, total])
            val_acc = correct / total
            val_accuracies.append(val_acc)
            metric = -val_acc
        else:
            metric = parallel.mean_over_ranks(avg_loss) if distributed else avg_loss
        if isinstance(scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
            scheduler.step(metric)
        elif scheduler is not None:
            scheduler.step()
        if abs(metric) >= best_val_acc:
            best_val_acc = abs(metric)
            parallel.broadcast_buffers(net)
            best_model_wts = (net.snapshot_state_dict() if hasattr(net, "snapshot_state_dict")
                              else copy.deepcopy(net.state_dict()))
            if e % save_epoch == 0:
                save_model(savename, net, camel_to_snake(str(net.__class__.__name__)), data_loader.dataset.name,
                           train_state="train", type="best_epoch", run=run, epoch=e, metric=abs(metric))
        if e == epoch:
            parallel.broadcast_buffers(net)
            save_model(savename, net, camel_to_snake(str(net.__class__.__name__)), data_loader.dataset.name,
                       train_state="train", type="final_epoch", run=run, epoch=e, metric=abs(metric))
        stats["epochs"].append({"seconds": time.perf_counter() - t_epoch, "batches": nb, "patches": npatch})
        stats["launch"] = stepper.launch
    stats["losses"] = losses
    return best_model_wts


def val(net, data_loader, device="cpu", supervision="full"):
    """model_utils.py:1135-1158: argmax accuracy over samples whose PREDICTION is not an ignored
    label.  Like the reference, the network is not switched to eval mode (it runs in whatever
    mode it is in — train mode when called from `train`).  The per-sample `.item()` loop becomes
    an on-device comparison with one host sync per batch."""
    correct, total = _val_counts(net, data_loader, device)
    return correct / total


def _val_counts(net, data_loader, device):
    """(correct, counted) of val(): the host counts, summed over ranks by train() under DP"""
    ignored = sorted(set(getattr(data_loader.dataset, "ignored_labels", [])))
    correct, total = 0, 0
    for data, data2, target in data_loader:
        with torch.no_grad():
            data, data2, target = data.to(device), data2.to(device), target.to(device)
            output = net(data, data2)
            if isinstance(output, tuple):
                output = output[0]
            pred = output.argmax(dim=1).view(-1)
            keep = torch.ones_like(pred, dtype=torch.bool)
            for lab in ignored:
                keep &= pred != lab
            correct += int(((pred == target.view(-1)) & keep).sum())
            total += int(keep.sum())
    return correct, total


def test(run, net, img1, img2, hyperparams):
    """Whole-image inference of model_utils.py:1067-1132 (center-pixel mode): eval-mode forward over
    every sliding window, probabilities accumulated at the window centres.  The image is uploaded
    once; windows are gathered on the device (vc_window_gather) and the logits scattered into an
    fp64 probability map on the device (vc_center_accumulate), so the Python generator + np.copy
    per window of the reference disappears.  Returns a float64 numpy array [W, H, n_classes] like
    the reference's `probs`.

    `hyperparams["border"]` (absent or None: as above; "symmetric", "reflect", "constant"): the run over the scene
    padded by patch_size // 2 in that np.pad mode and cut back -- restore_from_padding(test(padding_image(img1),
    padding_image(img2))), utils.py:320-354 -- with the padding folded into the gather's addresses, so pixels within
    patch_size // 2 of an edge get a probability row too."""
    return _runner(net, img1, img2, hyperparams).run(batch_size=hyperparams["batch_size"])


def predict(run, net, img1, img2, hyperparams, centers=None):
    """np.argmax(test(...), -1) (main.py:504) as an int64 [W, H] tensor on the device, without the probability map:
    each window's argmax is written at its centre (vc_center_argmax), 0 where no window was evaluated.  `centers`
    ([m, 2] integer scene pixels) evaluates only the windows centred there.  Needs test_stride 1 (ValueError)."""
    if hyperparams.get("test_stride", 1) != 1:
        raise ValueError(f"predict needs test_stride 1 (one window per centre), got {hyperparams['test_stride']}")
    return _runner(net, img1, img2, hyperparams).run_labels(centers=centers, batch_size=hyperparams["batch_size"])


def evaluate(run, net, img1, img2, gt, hyperparams):
    """The end of a run, main.py:500-519 -- test(), np.argmax, metrics() -- evaluating only what metrics() reads: the
    windows centred on the pixels of `gt` whose label is not in hyperparams["ignored_labels"].  The class map and the
    confusion counts stay on the device; the result is the reference's metrics dict.  Without a border it equals
    metrics(np.argmax(test(...), -1), gt, ignored_labels, n_classes): a labelled pixel within patch_size // 2 of an
    edge has no window and counts as predicted 0 there too; hyperparams["border"] gives those pixels windows.
    Needs test_stride 1 (ValueError)."""
    from . import metrics
    from .window import border_code
    if hyperparams.get("test_stride", 1) != 1:
        raise ValueError(f"evaluate needs test_stride 1 (one window per centre), got {hyperparams['test_stride']}")
    border_code(hyperparams.get("border"))
    gt = np.asarray(gt)
    ignored = list(hyperparams["ignored_labels"])
    centers = np.argwhere(~np.isin(gt, ignored))
    pred = predict(run, net, img1, img2, hyperparams, centers=centers)
    cm = metrics.confusion_matrix(pred, gt, ignored, hyperparams["n_classes"], device=pred.device)
    return metrics.scores(cm.cpu().numpy())


def _runner(net, img1, img2, hyperparams):
    """the SlidingWindowInference of test() / predict(): PCA as model_utils.py:1076-1077, window and border options"""
    from .window import border_code
    border_code(hyperparams.get("border"))     # an unknown mode is refused before any work
    net.eval()
    if hyperparams.get("applyPCA", False):
        pca, k = hyperparams.get("pca"), hyperparams.get("pca_components", 3)
        if pca is None:
            img1 = apply_pca(img1, k)   # model_utils.py:1076-1077 (3 components in the reference), on the host
        else:   # on the device; passing the training batcher's fitted `batcher.pca` shares one fit (pca.py)
            from .pca import resolve
            from .window import _cube
            img1 = resolve(pca, k, _cube(img1, torch.device(hyperparams["device"])))[1]
    return SlidingWindowInference(net, img1, img2, patch_size=hyperparams["patch_size"],
                                  step=hyperparams.get("test_stride", 1), n_classes=hyperparams["n_classes"],
                                  device=hyperparams["device"], border=hyperparams.get("border"))


def apply_pca(X, num_components):
    """utils.py:85-93 applyPCA: whitened PCA of the [W, H, C] cube's pixel spectra (host-side data
    preparation, as in the reference; sklearn's PCA)."""
    from sklearn.decomposition import PCA
    X = np.asarray(X)
    flat = np.reshape(X, (-1, X.shape[2]))
    flat = PCA(n_components=num_components, whiten=True).fit_transform(flat)
    return np.reshape(flat, (X.shape[0], X.shape[1], num_components))
