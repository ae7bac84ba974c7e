"""The MHST fixtures (tests/golden/gen_mhst_golden.py) and the model each was made with, shared by tests/test_mhst*.py."""
import torch

from helpers import grad_rule_fraction, load_case  # noqa: F401  (grad_rule_fraction: the tests import it from here)

REGISTRY = dict(patch_size=8, num_patches=64, encoder_embed_dim=64, en_heads=4, mlp_dim=8, dropout=0.1, emb_dropout=0.1,
                coefficient_hsi=0.6, coefficient_vit=0.7, hsp_vit_num_heads=16, head_tau=5, use_head_select=True,
                vit_qkv_bias=False, mlp_ratio=4, attnproj_mlp_drop=0.1, attn_drop=0.1)
CASES = {
    "mhst_a": dict(l1=30, l2=1, num_classes=16, en_depth=5, hsp_vit_depth=8),
    "mhst_b": dict(l1=11, l2=2, num_classes=12, en_depth=1, hsp_vit_depth=2),
}
_CACHE = {}


def load(name):
    """the fixture `name` (helpers.load_case), loaded once"""
    return load_case(name, _CACHE)


def build(name, p_zero=True):
    """the product model of a case, constructed under torch.manual_seed(0) as the fixture's was (CPU, train mode)"""
    from vitcnn_amd.mhst import MHST
    torch.manual_seed(0)
    m = MHST(**CASES[name], **REGISTRY)
    if p_zero:
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
    return m.train()
