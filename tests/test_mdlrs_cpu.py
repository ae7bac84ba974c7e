"""MDL-RS fusion CNNs, the checks that need no GPU: tests/mdlrs_oracle.py (float64) reproduces the reference modules'
own train logits, loss, every parameter gradient, BatchNorm running statistics, num_batches_tracked and eval logits
(tests/golden/mdlrs_*.npz, made by tests/golden/gen_mdlrs_golden.py from the reference's DML_Hong.py and losses.py,
with test_mft.py's oracle tolerances); the product modules construct without the HIP library and have the
reference's state_dict names, shapes and, seeded alike, initial values; get_model's defaults; constructor and
CPU-input rejections; and every new entry point (csrc/mdlrs.hip) returns 1 on bad arguments before any launch.
"""
import pytest
import torch

import mdlrs_oracle as O
from mdlrs_cases import CASES, N_KEYS, build, golden


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", list(CASES))
def test_mdlrs_oracle_matches_reference(name, dtype):
    """The restatement against the reference's own fp32 numbers, with test_mft.py's oracle tolerances.  Evaluated in
    fp32 it is compared like with like, and every quantity is held to them.  Evaluated in float64 (the form the GPU
    tests use) the logits, loss, running statistics and eval logits are held to them too; the gradients are not,
    because there the fixture's own fp32 error is what is measured: a conv bias in front of a train-mode BatchNorm has
    a true gradient of 0 and the fixture holds rounding noise up to 1.13e-6 (mdlrs_late_a conv1_b.bias), and
    mdlrs_cross_b's conv1_b.weight has an element off by 5.7e-6 at 3.7e-2.  The float64 gradients are held to a
    quarter of the fixtures' gradient rule (|g - g_ref| <= 1e-3 |g_ref| + 1e-5 gmax), which is what the generator
    guarantees for the reference's fp32 gradients against its own float64 run."""
    cls, case = CASES[name]
    sd, run, gr, t = golden(name)
    logits, loss, grads, running, _ = O.train_step(cls, sd, t["x1"], t["x2"], t["target"], t["weight"], dtype=dtype)
    logits = logits if isinstance(logits, tuple) else (logits,)
    assert len(logits) == len(t["logits"]) == (3 if cls == "Cross_fusion_CNN" else 1)
    for got, ref in zip(logits, t["logits"]):
        assert got.shape == (case["B"], case["ncls"])
        assert torch.allclose(got.float(), ref, rtol=1e-5, atol=1e-5)
    assert abs(float(loss) - t["loss"]) <= 1e-5 + 1e-5 * abs(t["loss"])
    assert set(grads) == set(gr) and len(sd) == N_KEYS[cls]
    gmax = max(float(g.double().norm()) for g in gr.values())
    for k, g in gr.items():
        if dtype == torch.float64:
            err = float((grads[k] - g.double()).norm())
            assert err <= 0.25 * (1e-3 * float(g.double().norm()) + 1e-5 * gmax), (k, err)
            continue
        assert torch.allclose(grads[k].float(), g, rtol=1e-4, atol=1e-6), (k, float((grads[k].float() - g).abs().max()))
    assert set(running) == set(run)
    for k, v in running.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(run[k]), k
        else:
            assert torch.allclose(v.float(), run[k], rtol=1e-5, atol=1e-6), k
    ev = O.eval_logits(cls, dict(sd, **run), t["x1"], t["x2"], dtype=dtype)
    ev = ev if isinstance(ev, tuple) else (ev,)
    for got, ref in zip(ev, t["eval_logits"]):
        assert torch.allclose(got.float(), ref, rtol=1e-5, atol=1e-5)


def test_cross_model_applies_its_shared_batchnorms_two_and_three_times():
    """what num_batches_tracked pins: bn4_a / bn4_b run twice per forward, bn5 / bn6 three times, the rest once"""
    _, run, _, _ = golden("mdlrs_cross_a")
    nbt = {k[:-len(".num_batches_tracked")]: int(v) for k, v in run.items() if k.endswith("num_batches_tracked")}
    assert nbt == {"bn1_a": 1, "bn2_a": 1, "bn3_a": 1, "bn4_a": 2, "bn1_b": 1, "bn2_b": 1, "bn3_b": 1, "bn4_b": 2,
                   "bn5": 3, "bn6": 3}


@pytest.mark.parametrize("name", list(CASES))
def test_mdlrs_constructs_without_the_library_with_the_reference_state_dict(name, monkeypatch):
    import vitcnn_amd.mdlrs as M

    def no_lib():
        raise AssertionError("constructing an MDL-RS model must not load the HIP library")

    monkeypatch.setattr(M, "lib", no_lib)
    cls, _ = CASES[name]
    sd, _, gr, _ = golden(name)
    torch.manual_seed(0)
    m = build(name)
    assert type(m).__name__ == cls
    mine = m.state_dict()
    assert list(mine.keys()) == list(sd.keys()) and len(mine) == N_KEYS[cls]
    for k in sd:
        assert mine[k].shape == sd[k].shape, k
        assert torch.equal(mine[k], sd[k]), k   # same creation order and initialisers -> the same draws
    assert [n for n, _ in m.named_parameters()] == list(gr.keys())
    m.load_state_dict({k: v + 1 for k, v in sd.items()})
    assert all(torch.equal(v, sd[k] + 1) for k, v in m.state_dict().items())


@pytest.mark.parametrize("cls", list(N_KEYS))
def test_get_model_mdlrs_defaults(cls):
    import vitcnn_amd
    from vitcnn_amd import AdamW, Cross_fusion_CNN_Loss, CrossEntropyLoss
    from vitcnn_amd.model_utils import REGISTERED, get_model
    assert cls in REGISTERED
    m, opt, crit, kw = get_model(cls, n_classes=16, n_bands=(144, 1), ignored_labels=[0], dataset="Houston2013",
                                 device=torch.device("cpu"))
    assert type(m) is getattr(vitcnn_amd, cls) and type(opt) is AdamW
    assert type(crit) is (Cross_fusion_CNN_Loss if cls == "Cross_fusion_CNN" else CrossEntropyLoss)
    assert kw["patch_size"] == 7 and kw["applyPCA"] is False and kw["lr"] == 1e-3 and kw["epoch"] == 150
    assert kw["batch_size"] == 64 and kw["center_pixel"] is True and kw["supervision"] == "full"
    g = opt.param_groups[0]
    assert g["lr"] == 1e-3 and g["weight_decay"] == 0.0 and g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8
    assert float(crit.weight[0]) == 0.0 and float(crit.weight[1]) == 1.0
    first = m.conv1 if cls == "Early_fusion_CNN" else m.conv1_a
    assert first.weight.shape == (16, 145 if cls == "Early_fusion_CNN" else 144, 3, 3)
    assert m.conv7.weight.shape == (16, 128 if cls == "Late_fusion_CNN" else 64, 1, 1)
    # applyPCA does not change n_bands for these four (model_utils.py:69-108)
    m2, _, _, kw2 = get_model(cls, n_classes=7, n_bands=(63, 2), ignored_labels=[0], dataset="x", applyPCA=True,
                              patch_size=9, device=torch.device("cpu"))
    assert m2.C1 == 63 and m2.C2 == 2 and kw2["applyPCA"] is True and kw2["patch_size"] == 9


def test_get_model_still_rejects_unknown_names():
    from vitcnn_amd.model_utils import get_model
    with pytest.raises(KeyError):
        get_model("Early_fusion", n_classes=16, n_bands=(144, 1), ignored_labels=[0], dataset="x")


@pytest.mark.parametrize("cls", list(N_KEYS))
def test_mdlrs_constructor_accepts_and_rejects(cls):
    from vitcnn_amd import mdlrs
    C = getattr(mdlrs, cls)
    for P in (5, 7, 8, 9, 11):
        C(30, 1, 16, patch_size=P)
    for c1, c2, n in ((1, 1, 2), (145, 8, 64), (512, 3, 20)):
        C(c1, c2, n)
    for bad in (dict(patch_size=2), dict(c2=0), dict(c1=0), dict(c1=513), dict(c2=9), dict(n=1), dict(n=65),
                dict(patch_size=33)):
        kw = dict(dict(c1=30, c2=1, n=16, patch_size=7), **bad)
        with pytest.raises(ValueError):
            C(kw["c1"], kw["c2"], kw["n"], patch_size=kw["patch_size"])
    with pytest.raises(ValueError):
        from vitcnn_amd.model_utils import get_model
        get_model(cls, n_classes=16, n_bands=(144, 1), ignored_labels=[0], dataset="x", patch_size=2,
                  device=torch.device("cpu"))


@pytest.mark.parametrize("name", ["mdlrs_early_b", "mdlrs_cross_b"])
def test_mdlrs_cpu_input_raises(name):
    m = build(name)
    with pytest.raises(RuntimeError):
        m(torch.zeros(2, 13, 5, 5), torch.zeros(2, 2, 5, 5))


def test_cross_fusion_loss_cpu_input_raises():
    from vitcnn_amd import Cross_fusion_CNN_Loss
    o = torch.zeros(2, 4)
    with pytest.raises(RuntimeError):
        Cross_fusion_CNN_Loss(weight=torch.ones(4))((o, o, o), torch.zeros(2, dtype=torch.int64))


def _raw():
    from vitcnn_amd._lib import lib
    return lib().raw


N = None
REJECTED = [
    ("pool C = 0", "vc_maxpool2p_fwd", (2, 7, 7, 0, N, 0, N, N, N, N, N, N, N)),
    ("pool ldx < C", "vc_maxpool2p_fwd", (2, 7, 7, 8, N, 7, N, N, N, N, N, N, N)),
    ("pool H < 2", "vc_maxpool2p_fwd", (2, 1, 7, 8, N, 8, N, N, N, N, N, N, N)),
    ("pool W < 2", "vc_maxpool2p_fwd", (2, 7, 1, 8, N, 8, N, N, N, N, N, N, N)),
    ("pool B < 0", "vc_maxpool2p_fwd", (-1, 7, 7, 8, N, 8, N, N, N, N, N, N, N)),
    ("pool with one of the four BatchNorm pointers", "vc_maxpool2p_fwd", (2, 7, 7, 8, N, 8, 16, N, N, N, N, N, N)),
    ("pool with three of the four BatchNorm pointers", "vc_maxpool2p_fwd", (2, 7, 7, 8, N, 8, 16, 16, N, 16, N, N, N)),
    ("pool without buffers", "vc_maxpool2p_fwd", (2, 7, 7, 8, N, 8, N, N, N, N, N, N, N)),
    ("pool past 2^31 elements", "vc_maxpool2p_fwd", (1 << 20, 64, 64, 8, 16, 8, N, N, N, N, 16, 16, N)),
    ("pool backward C = 0", "vc_maxpool2p_bwd", (2, 7, 7, 0, N, N, N, N, 0, N)),
    ("pool backward lddx < C", "vc_maxpool2p_bwd", (2, 7, 7, 8, N, N, N, N, 7, N)),
    ("pool backward H < 2", "vc_maxpool2p_bwd", (2, 1, 7, 8, N, N, N, N, 8, N)),
    ("pool backward without buffers", "vc_maxpool2p_bwd", (2, 7, 7, 8, N, N, N, N, 8, N)),
    ("head G = 4", "vc_avgpool_head_fwd", (3, 9, 64, 4, 16, 1, 16, 16, 16, 16, 16, 16, 16, N)),
    ("head G = 0", "vc_avgpool_head_fwd", (3, 9, 64, 0, 16, 0, 16, 16, 16, 16, 16, 16, 16, N)),
    ("head ncls = 0", "vc_avgpool_head_fwd", (3, 9, 64, 1, 0, 0, 16, N, N, 16, 16, 16, 16, N)),
    ("head C = 0", "vc_avgpool_head_fwd", (3, 9, 0, 1, 16, 0, 16, N, N, 16, 16, 16, 16, N)),
    ("head C = 1025", "vc_avgpool_head_fwd", (3, 9, 1025, 1, 16, 0, 16, N, N, 16, 16, 16, 16, N)),
    ("head HW = 0", "vc_avgpool_head_fwd", (3, 0, 64, 1, 16, 0, 16, N, N, 16, 16, 16, 16, N)),
    ("head B = 0", "vc_avgpool_head_fwd", (0, 9, 64, 1, 16, 0, 16, N, N, 16, 16, 16, 16, N)),
    ("head mode = 2", "vc_avgpool_head_fwd", (3, 9, 64, 2, 16, 2, 16, 16, N, 16, 16, 16, 16, N)),
    ("head G = 2 without the second map", "vc_avgpool_head_fwd", (3, 9, 64, 2, 16, 0, 16, N, N, 16, 16, 16, 16, N)),
    ("head backward G = 4", "vc_avgpool_head_bwd", (3, 9, 64, 4, 16, 1, 16, 16, 16, 16, 16, 16, 16, 16, N)),
    ("head backward ncls = 0", "vc_avgpool_head_bwd", (3, 9, 64, 1, 0, 0, 16, 16, 16, 16, N, N, 16, 16, N)),
    ("head backward G = 3 without the third gradient", "vc_avgpool_head_bwd",
     (3, 9, 64, 3, 16, 1, 16, 16, 16, 16, 16, N, 16, 16, N)),
    ("head backward without dW", "vc_avgpool_head_bwd", (3, 9, 64, 1, 16, 0, 16, 16, 16, 16, N, N, N, 16, N)),
    ("loss B = 0", "vc_xfusion_loss_fwd_bwd", (0, 16, 16, 16, 16, 16, N, 16, 16, 16, 16, N)),
    ("loss ncls = 0", "vc_xfusion_loss_fwd_bwd", (4, 0, 16, 16, 16, 16, N, 16, 16, 16, 16, N)),
    ("loss without the third logits", "vc_xfusion_loss_fwd_bwd", (4, 16, 16, 16, N, 16, N, 16, 16, 16, 16, N)),
    ("loss without a gradient buffer", "vc_xfusion_loss_fwd_bwd", (4, 16, 16, 16, 16, 16, N, 16, 16, N, 16, N)),
]


@pytest.mark.parametrize("what,name,args", REJECTED, ids=[r[0] for r in REJECTED])
def test_mdlrs_host_side_rejections(what, name, args):
    """VC_REQUIRE returns 1 (hipErrorInvalidValue) before any launch: the pointers (null, or the never-dereferenced
    address 16) are not touched and no GPU is needed"""
    assert _raw()[name](*args) == 1, what
