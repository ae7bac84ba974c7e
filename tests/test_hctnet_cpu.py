"""HCTnet comparison model without a GPU: tests/hct_oracle.py (float64, torch functional ops) reproduces the reference
module's own train logits, loss, every parameter gradient, BatchNorm running statistics and eval logits
(tests/golden/hctnet_a*.npz, hctnet_b*.npz, made by tests/golden/gen_hctnet_golden.py from the reference's HCTnet.py);
the product module constructs without the HIP library and has the reference's 77 state_dict names in order, their
shapes and, seeded alike, initial values; get_model("HCTnet") gives the reference's defaults; the constructor and
forward reject what the kernels cannot take.  Tolerances are test_mft.py's.
"""
import numpy as np
import pytest
import torch

import hct_oracle as O
from hct_cases import KW, UNUSED, golden


@pytest.mark.parametrize("name", list(KW))
def test_hct_oracle_matches_reference(name):
    sd, run, gr, t = golden(name)
    logits, loss, grads, running, pre = O.train_step(sd, t["x1"], t["x2"], t["target"], t["weight"])
    assert torch.allclose(logits.float(), t["logits"], rtol=1e-5, atol=1e-5)
    assert abs(float(loss) - t["loss"]) <= 1e-5 + 1e-5 * abs(t["loss"])
    assert set(grads) == set(gr) and len(sd) == 77 and len(gr) == 68
    for k, g in gr.items():
        assert torch.allclose(grads[k].float(), g, rtol=1e-4, atol=1e-6), (k, float((grads[k].float() - g).abs().max()))
    unused = [k for k in gr if k.startswith(UNUSED)]
    assert len(unused) == 12
    for k in unused:
        assert not gr[k].any() and not grads[k].any(), k
    assert len(running) == 6 and len(pre) == 3
    for k, v in running.items():
        assert torch.allclose(v.float(), run[k], rtol=1e-5, atol=1e-6), k
    assert min(float(v.abs().min()) for v in pre.values()) >= 1e-5   # the generator's first seed condition
    after = dict(sd, **run)
    assert torch.allclose(O.eval_logits(after, t["x1"], t["x2"]).float(), t["eval_logits"], rtol=1e-5, atol=1e-5)


def test_hct_oracle_dropout_sites():
    """the drop dictionary covers the 12 sites, and every one of them changes the logits"""
    sd, _, _, t = golden("hctnet_b")
    assert len(O.SITES) == 12
    B, T = 4, 5
    shapes = {"emb": (B, T, 64), "attn": (B, T, 64), "ff1": (B, T, 8), "ff2": (B, T, 64), "prob": (B, 8, 1, T),
              "out": (B, 1, 64)}
    base = O.eval_logits(sd, t["x1"], t["x2"])
    g = torch.Generator().manual_seed(0)
    for site in O.SITES:
        kind = "emb" if site.startswith("emb") else site.rsplit(".", 1)[1]
        mask = (torch.rand(shapes[kind], generator=g) >= 0.5).double()
        P = {k: v.double() if O.is_param(k) else v for k, v in sd.items()}
        with torch.no_grad():
            got = O.forward(P, t["x1"].double(), t["x2"].double(), False, {site: (mask, 0.5)})
        assert float((got - base).abs().max()) > 1e-6, site


@pytest.mark.parametrize("name", list(KW))
def test_hctnet_constructs_without_the_library_with_the_reference_state_dict(name, monkeypatch):
    import vitcnn_amd.hctnet as M

    def no_lib():
        raise AssertionError("constructing HCTnet must not load the HIP library")

    monkeypatch.setattr(M, "lib", no_lib)
    sd, _, gr, _ = golden(name)
    torch.manual_seed(0)
    m = M.HCTnet(**KW[name])
    mine = m.state_dict()
    assert list(mine.keys()) == list(sd.keys()) and len(mine) == 77
    for k in sd:
        assert mine[k].shape == sd[k].shape, k
        assert torch.equal(mine[k], sd[k]), k   # same creation order and initialisers -> the same draws
    assert [n for n, _ in m.named_parameters()] == list(gr.keys())
    # the four packed blocks the fused kernels read are contiguous, 16-B aligned, and hold what the names say
    assert set(m._packed) == {"enc0", "enc1", "ct0", "ct1"} and all(o % 4 == 0 for o in m._packed.values())
    flat = m.flat_params.detach()
    o = m._packed["ct1"]
    wq = mine["fusion_encoder.layers.0.2.layers.0.1.fn.fn.to_q.weight"]
    assert torch.equal(flat[o + 128:o + 128 + wq.numel()].view(wq.shape), wq)
    o = m._packed["enc0"]
    w2 = mine["fusion_encoder.layers.0.0.layers.0.1.fn.fn.net.3.weight"]
    assert torch.equal(flat[o + 17416:o + 17416 + 512].view(64, 8), w2)


def test_hctnet_default_constructor_is_the_references():
    from vitcnn_amd.hctnet import HCTnet
    m = HCTnet()
    assert m.mlp_head[1].weight.shape == (6, 64) and m.token_wA.shape == (1, 4, 64)
    assert m.pos_embedding.shape == (1, 5, 64) and m.dropout.p == 0.1
    assert m.conv3d_features[0].weight.shape == (8, 1, 3, 3, 3) and m.conv2d_features2[0].weight.shape == (64, 1, 3, 3)
    att = m.fusion_encoder.layers[0][2].layers[0][0].fn.fn
    assert att.to_kv.weight.shape == (1024, 64) and att.to_q.bias is None and att.dropout.p == 0.1
    assert m.fusion_encoder.layers[0][0].layers[0][0].fn.fn.scale == 0.125


def test_hctnet_constructor_rejects_unsupported_shapes():
    from vitcnn_amd.hctnet import HCTnet
    bad = (dict(num_tokens=0), dict(num_tokens=9), dict(dim=32), dict(h_dim=32), dict(l_dim=128), dict(depth=2),
           dict(h_enc_depth=2), dict(l_enc_depth=2), dict(ct_attn_depth=2), dict(ct_attn_dim_head=32),
           dict(h_enc_heads=4), dict(l_enc_heads=4), dict(ct_attn_heads=4), dict(h_enc_mlp_dim=16),
           dict(l_enc_mlp_dim=16), dict(num_classes=0), dict(in_channels=0), dict(dropout=1.0))
    for kw in bad:
        with pytest.raises(ValueError):
            HCTnet(**kw)
    for L in (1, 8):
        assert HCTnet(num_tokens=L).pos_embedding.shape == (1, L + 1, 64)


def test_get_model_hctnet_defaults():
    from vitcnn_amd import AdamW, CrossEntropyLoss, HCTnet
    from vitcnn_amd.model_utils import REGISTERED, get_model
    assert "HCTnet" in REGISTERED
    m, opt, crit, kw = get_model("HCTnet", n_classes=16, n_bands=(144, 1), ignored_labels=[0], dataset="Houston2013",
                                 device=torch.device("cpu"))
    assert type(m) is HCTnet and type(opt) is AdamW and type(crit) is CrossEntropyLoss
    assert kw["patch_size"] == 11 and kw["applyPCA"] is True and kw["lr"] == 1e-4 and kw["epoch"] == 100
    assert kw["batch_size"] == 64 and kw["center_pixel"] is True and kw["supervision"] == "full"
    g = opt.param_groups[0]
    assert g["lr"] == 1e-4 and g["weight_decay"] == 0.0 and g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8
    assert m.L == 6 and m.ncls == 16 and m.in_channels == 1 and len(m.state_dict()) == 77
    assert float(crit.weight[0]) == 0.0 and float(crit.weight[1]) == 1.0
    _, _, _, kw2 = get_model("HCTnet", n_classes=7, n_bands=(63, 1), ignored_labels=[0], dataset="x", applyPCA=False,
                             device=torch.device("cpu"))
    assert kw2["applyPCA"] is False


def test_hctnet_cpu_input_raises():
    from vitcnn_amd.hctnet import HCTnet
    m = HCTnet(**KW["hctnet_b"])
    with pytest.raises(RuntimeError):
        m(torch.zeros(2, 3, 7, 7), torch.zeros(2, 1, 7, 7))


def test_patchbatcher_signature_has_apply_pca():
    import inspect

    from vitcnn_amd.window import PatchBatcher
    p = inspect.signature(PatchBatcher.__init__).parameters["applyPCA"]
    assert p.default is False and p.annotation in (bool, "bool")


def test_fixture_files_are_under_the_size_limit():
    import glob
    import os

    from hct_cases import HERE
    files = glob.glob(os.path.join(HERE, "golden", "hctnet_*.npz"))
    assert len(files) == 12
    assert all(os.path.getsize(f) < (1 << 20) for f in files)
    assert np.load(os.path.join(HERE, "golden", "hctnet_a.npz"))["seed"] == 2
