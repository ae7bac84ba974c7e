"""vitcnn_amd — MI355X-native ViT-CNN ("Multimodality_Mamba") training hot path.

Python mirror of the reference's plugin surface (model_utils.get_model / train / test / val)
over hand-written gfx950 HIP kernels behind the C ABI in include/vitcnn.h.
"""
from .model import Multimodality_Mamba  # noqa: F401
from .losses import Cross_fusion_CNN_Loss, CrossEntropyLoss, EndNet_Loss, GLT_Loss  # noqa: F401
from .optim import Adam, AdamW  # noqa: F401
from .step import fused_train_step  # noqa: F401
from .mft import MFT  # noqa: F401
from .mdlrs import Cross_fusion_CNN, Early_fusion_CNN, Late_fusion_CNN, Middle_fusion_CNN  # noqa: F401
from .endnet import EndNet  # noqa: F401
from .spectralformer import SpectralFormer  # noqa: F401
from .hctnet import HCTnet  # noqa: F401
from .s2eft import S2EFT  # noqa: F401
from .mhst import MHST  # noqa: F401
from .glt import GLT  # noqa: F401
from .model_utils import evaluate, predict, test  # noqa: F401  (the end of a run: main.py:500-519)

__all__ = ["Multimodality_Mamba", "CrossEntropyLoss", "Cross_fusion_CNN_Loss", "AdamW", "Adam", "MFT", "Early_fusion_CNN",
           "Middle_fusion_CNN", "Late_fusion_CNN", "Cross_fusion_CNN", "EndNet", "SpectralFormer", "HCTnet",
           "S2EFT", "MHST", "GLT", "EndNet_Loss", "GLT_Loss", "fused_train_step", "test", "predict", "evaluate"]
