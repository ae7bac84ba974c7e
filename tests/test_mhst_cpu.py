"""MHST comparison model without a GPU: tests/mhst_oracle.py (float64, torch functional ops, fed the recorded gate noise)
reproduces the reference's float64 twin -- train output, loss, every parameter gradient, BatchNorm running statistics,
eval output (tests/golden/mhst_a*.npz, mhst_b*.npz, made by tests/golden/gen_mhst_golden.py from the reference's
MHST/ modules); the product module has the reference's state_dict names in order, their shapes and, seeded alike, initial
values; get_model("MHST") gives the reference's defaults; construction, forward and the new entry points reject what the
kernels cannot take, on the host.

Bounds: output and loss 1e-9 relative, gradients 1e-6 of their norm (float64 against float64 values, the gradients
stored in fp32: consistency bounds)."""
import numpy as np
import pytest
import torch

import mhst_oracle as O
from mhst_cases import CASES, REGISTRY, build, load


@pytest.mark.parametrize("name", list(CASES))
def test_mhst_oracle_matches_reference(name):
    t = load(name)
    out, loss, grads, rec = O.train_step(t["state"], t["x1"], t["x2"], t["target"], t["weight"], t["noise"])
    ref = t["out"].double()
    assert float((out - ref).abs().max()) <= 1e-9 * float(ref.abs().max())
    assert abs(float(loss) - float(t["loss"])) <= 1e-9 * abs(float(t["loss"]))
    assert set(grads) == set(t["grads"])
    for k, g in t["grads"].items():
        err = float((grads[k] - g.double()).norm())
        assert err <= 1e-6 * float(g.double().norm()) + 1e-12, (k, err)
    assert set(rec["running"]) == set(t["running"])
    for k, v in t["running"].items():
        assert torch.allclose(rec["running"][k].float(), v, rtol=1e-6, atol=1e-7), k
    # the generator's seed conditions hold for the oracle's own intermediates
    assert min(float(v.abs().min()) for v in rec["pre"].values()) >= 1e-5
    assert min(float(v.abs().min()) for v in rec["gate"].values()) >= 1e-3 / O.TAU
    after = dict(t["state"], **t["running"])
    rec2 = {}
    ev = O.eval_forward(after, t["x1"], t["x2"], rec2)
    assert float((ev - t["eval_out"].double()).abs().max()) <= 1e-6 * float(t["eval_out"].abs().max())
    assert min(float(v.abs().min()) for v in rec2["gate"].values()) >= 1e-3


def test_mhst_oracle_noise_and_dropout_sites_matter():
    t = load("mhst_b")
    P = {k: v.double() for k, v in t["state"].items()}
    assert O.depths(P) == (1, 2) and len(O.sites(P)) == 1 + 3 + 8
    with torch.no_grad():
        base = O.forward(P, t["x1"].double(), t["x2"].double(), True, noise=t["noise"])
        flipped = O.forward(P, t["x1"].double(), t["x2"].double(), True, noise=-50.0 * torch.ones_like(t["noise"]))
        assert float((base - flipped).abs().max()) > 1e-6
        g = torch.Generator().manual_seed(0)
        shapes = {"emb": (3, 65, 64), "attn": (3, 65, 64), "ff1": (3, 65, 8), "ff2": (3, 65, 64),
                  "prob": (3, 16, 65, 65), "proj": (3, 65, 64), "fc1": (3, 65, 256), "fc2": (3, 65, 64)}
        for site in O.sites(P):
            mask = (torch.rand(shapes[site.rsplit(".", 1)[-1]], generator=g) >= 0.5).double()
            got = O.forward(P, t["x1"].double(), t["x2"].double(), True, noise=t["noise"], drop={site: (mask, 0.5)})
            assert float((got - base).abs().max()) > 1e-9, site


@pytest.mark.parametrize("name", list(CASES))
def test_mhst_has_the_reference_state_dict(name):
    t = load(name)
    m = build(name)
    sd = m.state_dict()
    assert list(sd) == t["keys"]
    assert len(sd) == (338 if name == "mhst_a" else 150)
    for k, v in t["state"].items():
        assert sd[k].shape == v.shape, k
        if v.dtype.is_floating_point:
            assert torch.equal(sd[k], v), k     # the same seed draws the same values, bit for bit
    if name == "mhst_a":
        assert sum(p.numel() for p in m.parameters()) == 737740


def test_get_model_mhst_defaults():
    import vitcnn_amd
    from vitcnn_amd import model_utils as mu
    assert "MHST" in mu.REGISTERED and vitcnn_amd.MHST is not None
    model, opt, crit, kw = mu.get_model("MHST", n_classes=16, n_bands=(144, 1), ignored_labels=[0], dataset="Houston2013",
                                        device=torch.device("cpu"))
    assert isinstance(model, vitcnn_amd.MHST) and len(model.state_dict()) == 338
    assert sum(p.numel() for p in model.parameters()) == 1164556
    assert (kw["patch_size"], kw["epoch"], kw["batch_size"], kw["lr"], kw["applyPCA"]) == (8, 1000, 64, 8e-4, False)
    assert kw["center_pixel"] is True and "pca_components" not in kw
    assert isinstance(opt, vitcnn_amd.AdamW) and isinstance(crit, vitcnn_amd.CrossEntropyLoss)
    assert float(crit.weight[0]) == 0.0 and float(crit.weight[1]) == 1.0
    blk = model.HeadSelectViT.blocks[0]
    assert (model.dropout.p, blk.attn.attn_drop.p, blk.attn.proj_drop.p, blk.mlp.drop.p) == (0.1, 0.1, 0.1, 0.1)
    assert float(model.weight_hsi.detach()) == pytest.approx(0.6) and float(model.vit_cls_coefficient.detach()) == pytest.approx(0.7)
    model, _, _, kw = mu.get_model("MHST", n_classes=16, n_bands=(144, 1), ignored_labels=[0], dataset="Houston2013",
                                   device=torch.device("cpu"), applyPCA=True)
    assert kw["pca_components"] == 30 and model.l1 == 30
    assert sum(p.numel() for p in model.parameters()) == 737740


@pytest.mark.parametrize("bad", [dict(patch_size=9), dict(encoder_embed_dim=32), dict(en_heads=8), dict(hsp_vit_num_heads=8),
                                 dict(vit_qkv_bias=True), dict(use_head_select=False), dict(dropout=1.0),
                                 dict(head_tau=0)])
def test_mhst_rejects_at_construction(bad):
    from vitcnn_amd.mhst import MHST
    kw = dict(CASES["mhst_b"], **REGISTRY)
    kw.update(bad)
    with pytest.raises(ValueError):
        MHST(**kw)


def test_mhst_rejects_bad_bands_and_classes():
    from vitcnn_amd.mhst import MHST
    for bad in (dict(l1=0), dict(l2=0), dict(num_classes=0), dict(num_classes=257)):
        with pytest.raises(ValueError):
            MHST(**dict(dict(CASES["mhst_b"], **REGISTRY), **bad))


def test_mhst_forward_rejects_cpu_inputs():
    m = build("mhst_b")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(3, 11, 8, 8), torch.zeros(3, 2, 8, 8))


def _raw():
    from vitcnn_amd._lib import lib
    return lib().raw


N = None   # every pointer is null: should a check ever let a call through, nothing can be touched
CONV_OK = (1, 4, 8, 8, 16, 16, 1, 3, 3, 1, 1, 4)
REJECTED = [
    ("conv even kernel", "vc_mhst_conv_fwd", (1, 4, 8, 8, 16, 16, 1, 3, 4, 1, 1, 4, N, 16, N, N, N, 16, N)),
    ("conv kernel 11", "vc_mhst_conv_fwd", (1, 4, 8, 8, 16, 16, 1, 3, 11, 1, 1, 4, N, 16, N, N, N, 16, N)),
    ("conv C not divisible by G", "vc_mhst_conv_fwd", (1, 1, 8, 8, 18, 16, 4, 1, 3, 1, 0, 1, N, 18, N, N, N, 16, N)),
    ("conv wrong Dout", "vc_mhst_conv_fwd", (1, 10, 8, 8, 1, 16, 1, 11, 3, 3, 5, 5, N, 1, N, N, N, 16, N)),
    ("conv ldx < C", "vc_mhst_conv_fwd", CONV_OK + (N, 15, N, N, N, 16, N)),
    ("conv ldy < O", "vc_mhst_conv_fwd", CONV_OK + (N, 16, N, N, N, 15, N)),
    ("conv null operands", "vc_mhst_conv_fwd", CONV_OK + (N, 16, N, N, N, 16, N)),
    ("dgrad lddx < C", "vc_mhst_conv_dgrad", CONV_OK + (N, 16, N, N, 15, 0.0, N)),
    ("dgrad B = 0", "vc_mhst_conv_dgrad", (0,) + CONV_OK[1:] + (N, 16, N, N, 16, 0.0, N)),
    ("wgrad lddy < O", "vc_mhst_conv_wgrad", CONV_OK + (N, 16, N, 15, N, N, N)),
    ("wgrad stride 0", "vc_mhst_conv_wgrad", (1, 4, 8, 8, 16, 16, 1, 3, 3, 0, 1, 4, N, 16, N, 16, N, N, N)),
    ("conv3 D = 0", "vc_mhst_conv3_fwd", (1, 0, N, 16, N, N, N, 16, N)),
    ("conv3 ldx < 16", "vc_mhst_conv3_fwd", (1, 2, N, 12, N, N, N, 16, N)),
    ("conv3 null operands", "vc_mhst_conv3_fwd", (1, 2, N, 16, N, N, N, 16, N)),
    ("conv3 dgrad lddx < 16", "vc_mhst_conv3_dgrad", (1, 2, N, 16, N, N, 15, 0.0, N)),
    ("conv3 wgrad without a workspace", "vc_mhst_conv3_wgrad", (1, 2, N, 16, N, 16, N, N, 0, N)),
    ("embed B = 0", "vc_mhst_embed_fwd", (0, N, N, N, N, N, N, N, N, N, N, N)),
    ("embed null operands", "vc_mhst_embed_fwd", (1, N, N, N, N, N, N, N, N, N, N, N)),
    ("embed_bwd null operands", "vc_mhst_embed_bwd", (1, N, N, N, N, N, N, N, N, N, N, N)),
    ("gate ldx < 64", "vc_mhst_gate_fwd", (1, N, 63, N, N, N, 1, 5.0, 0, N, N, N, N, N)),
    ("gate tau = 0", "vc_mhst_gate_fwd", (1, N, 64, N, N, N, 1, 0.0, 0, N, N, N, N, N)),
    ("gate train = 2", "vc_mhst_gate_fwd", (1, N, 64, N, N, N, 2, 5.0, 0, N, N, N, N, N)),
    ("gate_ds without a seed", "vc_mhst_gate_fwd_ds", (1, N, 64, N, N, N, 1, 5.0, N, 0, N, N, N, N, N)),
    ("gate_bwd null operands", "vc_mhst_gate_bwd", (1, N, N, 0.2, N, N)),
    ("headmask T = 64", "vc_mhst_headmask_fwd", (1, 64, 64, N, N, N, N)),
    ("headmask width 128", "vc_mhst_headmask_fwd", (1, 65, 128, N, N, N, N)),
    ("headmask_bwd width 128", "vc_mhst_headmask_bwd", (1, 65, 128, N, N, N, N, N, 0.0, N)),
    ("pool eps = 0", "vc_mhst_pool_fwd", (1, N, N, 0.0, N, N)),
    ("pool_bwd B = 0", "vc_mhst_pool_bwd", (0, N, N, 1e-5, N, N, N, N)),
    ("attn p = 1", "vc_mhst_attn_fwd", (1, N, 0.5, 1.0, 0, N, N, N)),
    ("attn p > 0 without a mask", "vc_mhst_attn_fwd", (1, N, 0.5, 0.1, 0, N, N, N)),
    ("attn B past the 32-bit mask index", "vc_mhst_attn_fwd", (40000, N, 0.5, 0.0, 0, N, N, N)),
    ("attn_ds without a seed", "vc_mhst_attn_fwd_ds", (1, N, 0.5, 0.0, N, 0, N, N, N)),
    ("attn_bwd p > 0 without a mask", "vc_mhst_attn_bwd", (1, N, 0.5, 0.1, N, N, N, N)),
    ("hsattn ldx < 64", "vc_mhst_hsattn_fwd", (1, N, 63, N, N, N, 1, 5.0, 0, 0, N, N, 1e-5, 0.5, 0.0, N, N, N, N, N, N, N)),
    ("hsattn p = 1", "vc_mhst_hsattn_fwd", (1, N, 64, N, N, N, 1, 5.0, 0, 0, N, N, 1e-5, 0.5, 1.0, N, N, N, N, N, N, N)),
    ("hsattn_ds without a seed", "vc_mhst_hsattn_fwd_ds", (1, N, 64, N, N, N, 1, 5.0, N, 0, 0, N, N, 1e-5, 0.5, 0.0, N, N, N,
                                                          N, N, N, N)),
    ("hsattn_bwd eps = 0", "vc_mhst_hsattn_bwd", (1, N, N, N, N, 0.0, 0.5, 0.0, N, N, N, 0.2, N, N, N, N)),
    ("tail ncls = 257", "vc_mhst_tail_fwd", (1, 257, N, N, 32, N, N, N, N, N, N, N, N, N)),
    ("tail ldz < 32", "vc_mhst_tail_fwd", (1, 16, N, N, 31, N, N, N, N, N, N, N, N, N)),
    ("tail_bwd ncls = 0", "vc_mhst_tail_bwd", (1, 0, N, N, N, N, N, N, N, N, N, 32, N, N)),
]


@pytest.mark.parametrize("what,name,args", REJECTED, ids=[r[0] for r in REJECTED])
def test_mhst_host_side_rejections(what, name, args):
    """VC_REQUIRE returns 1 (hipErrorInvalidValue) before any launch"""
    assert _raw()[name](*args) == 1, what


def test_conv3_workspace_query():
    from vitcnn_amd._lib import lib
    assert lib().vc_mhst_conv3_wgrad_ws_floats(4, 10) == 40 * 6912
    assert lib().vc_mhst_conv3_wgrad_ws_floats(64, 48) == 512 * 6912
    assert _raw()["vc_mhst_conv3_wgrad_ws_floats"](0, 3) == -1


def test_fixture_sizes():
    import glob
    import os
    from helpers import GOLDEN
    files = glob.glob(os.path.join(GOLDEN, "mhst_*.npz"))
    assert len(files) == 14
    assert all(os.path.getsize(f) < (1 << 20) for f in files)
    assert sum(os.path.getsize(f) for f in files) < (8 << 20)
    assert int(np.asarray(load("mhst_a")["seed"])) == 7 and int(np.asarray(load("mhst_b")["seed"])) == 4
