"""The GLT-Net fixtures (tests/golden/gen_glt_golden.py) and the model each was made with, shared by tests/test_glt*.py."""
import torch

from helpers import grad_rule_fraction, load_case  # noqa: F401  (grad_rule_fraction: the tests import it from here)

REGISTRY = dict(encoder_embed_dim=64, decoder_embed_dim=32, en_heads=4, de_heads=4, mlp_dim=8, dim_head=16, dropout=0.1,
                emb_dropout=0.1)
CASES = {
    "glt_a": dict(l1=30, l2=1, patch_size=8, num_patches=64, num_classes=16, en_depth=5, de_depth=5),
    "glt_b": dict(l1=11, l2=2, patch_size=4, num_patches=16, num_classes=12, en_depth=1, de_depth=2),
}
_CACHE = {}


def load(name):
    """the fixture `name` (helpers.load_case), loaded once"""
    return load_case(name, _CACHE)


def build(name, p_zero=True):
    """the product model of a case, constructed under torch.manual_seed(0) as the fixture's was (CPU, train mode)"""
    from vitcnn_amd.glt import GLT
    torch.manual_seed(0)
    m = GLT(**CASES[name], **REGISTRY)
    if p_zero:
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
    return m.train()
