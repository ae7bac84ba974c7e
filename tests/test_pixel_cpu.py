"""EndNet and SpectralFormer, the checks that need no GPU: tests/pixel_oracle.py reproduces the reference modules' own
train outputs, loss, every parameter gradient, BatchNorm running statistics, num_batches_tracked and eval outputs
(tests/golden/endnet_*.npz, spectralformer_*.npz, made by tests/golden/gen_pixel_golden.py from the reference's
EndNet.py, spectralformer.py and losses.py, with test_mft.py's oracle tolerances); the product modules construct
without the HIP library and have the reference's state_dict names, shapes and, seeded alike, initial values;
get_model's defaults; constructor, CPU-input and B = 1 rejections; and every new entry point (csrc/pixel.hip) returns
1 on bad arguments before any launch.
"""
import pytest
import torch

import pixel_oracle as O
from pixel_cases import CASES, N_KEYS, build, golden


def _oracle_step(cls, sd, t, dtype):
    if cls == "EndNet":
        return O.endnet_train_step(sd, t["x1"], t["x2"], t["target"], t["weight"], dtype=dtype)
    logits, loss, grads = O.sf_train_step(sd, t["x1"], t["x2"], t["target"], t["weight"], dtype=dtype)
    return (logits,), loss, grads, {}, {}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", list(CASES))
def test_pixel_oracle_matches_reference(name, dtype):
    """The restatement against the reference's own fp32 numbers, with test_mft.py's oracle tolerances: outputs, loss
    and eval outputs rtol 1e-5 / atol 1e-5, gradients rtol 1e-4 / atol 1e-6 (the zero-gradient Linear biases in front
    of a train-mode BatchNorm included), running statistics rtol 1e-5 / atol 1e-6.  SpectralFormer is held to them
    evaluated in fp32 and in float64; EndNet evaluated in fp32, like with like.

    EndNet evaluated in float64 (the form the GPU tests use) measures the fixture's own fp32 error: six train-mode
    BatchNorms over B = 3 or 4 rows stand in front of its logits, and the reference's fp32 logits sit up to 2.4e-5
    from float64 (endnet_b), its gradients at up to 0.26 of the fixtures' gradient rule.  The GPU tests hold the HIP
    path to that rule against the fixture (outputs 1e-3 relative; |g - g_ref| <= 1e-3 |g_ref| + 1e-5 gmax; running
    statistics rtol 1e-3 / atol 1e-4), which budgets the fixture's fp32 error and the kernels' together, so EndNet's
    float64 run has to leave the kernels half of each: its bounds are half the GPU rule."""
    cls, case = CASES[name]
    sd, run, gr, t = golden(name)
    fp32 = dtype == torch.float32 or cls == "SpectralFormer"     # "held to test_mft.py's tolerances"
    outs, loss, grads, running, _ = _oracle_step(cls, sd, t, dtype)
    assert len(outs) == len(t["outs"]) == (3 if cls == "EndNet" else 1)
    assert outs[0].shape == (case["B"], case["ncls"])

    def check_outs(got_all, ref_all):
        for got, ref in zip(got_all, ref_all):
            assert got.shape == ref.shape
            if fp32:
                assert torch.allclose(got.float(), ref, rtol=1e-5, atol=1e-5)
            else:
                assert _rel(got, ref) <= 0.5e-3, _rel(got, ref)

    check_outs(outs, t["outs"])
    assert abs(float(loss) - t["loss"]) <= ((1e-5 + 1e-5 * abs(t["loss"])) if fp32 else 0.5e-3 * abs(t["loss"]))
    assert set(grads) == set(gr) and len(sd) == N_KEYS[cls]
    gmax = max(float(g.double().norm()) for g in gr.values())
    for k, g in gr.items():
        if fp32:
            assert torch.allclose(grads[k].float(), g, rtol=1e-4, atol=1e-6), (k, float((grads[k].float() - g).abs().max()))
        else:
            err = float((grads[k] - g.double()).norm())
            assert err <= 0.5 * (1e-3 * float(g.double().norm()) + 1e-5 * gmax), (k, err)
    assert set(running) == set(run)
    for k, v in running.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(run[k]), k
        elif fp32:
            assert torch.allclose(v.float(), run[k], rtol=1e-5, atol=1e-6), k
        else:
            assert torch.allclose(v.float(), run[k], rtol=0.5e-3, atol=0.5e-4), k
    if cls == "EndNet":
        ev = O.endnet_eval(dict(sd, **run), t["x1"], t["x2"], dtype=dtype)
    else:
        ev = (O.sf_eval(sd, t["x1"], t["x2"], dtype=dtype),)
    check_outs(ev, t["eval_outs"])


def test_the_fixtures_pin_the_parameters_the_forward_never_applies():
    """joint_encoder_bn7 (EndNet.py:46, never applied at :76): zero gradient, counter 0, initial running statistics,
    while each of the other ten BatchNorms counts 1; SpectralFormer's skipcat convolutions ('ViT' mode): zero gradient"""
    _, run, gr, _ = golden("endnet_a")
    nbt = {k[:-len(".num_batches_tracked")]: int(v) for k, v in run.items() if k.endswith("num_batches_tracked")}
    assert len(nbt) == 11 and nbt.pop("joint_encoder_bn7") == 0 and set(nbt.values()) == {1}
    assert not run["joint_encoder_bn7.running_mean"].any() and bool((run["joint_encoder_bn7.running_var"] == 1).all())
    assert not gr["joint_encoder_bn7.weight"].any() and not gr["joint_encoder_bn7.bias"].any()
    _, _, gr, _ = golden("spectralformer_a")
    skip = [k for k in gr if k.startswith("transformer.skipcat.")]
    assert len(skip) == 6 and not any(gr[k].any() for k in skip)


@pytest.mark.parametrize("name", list(CASES))
def test_pixel_models_construct_without_the_library_with_the_reference_state_dict(name, monkeypatch):
    import vitcnn_amd.endnet as E
    import vitcnn_amd.s2eft as S

    def no_lib():
        raise AssertionError("constructing a per-pixel model must not load the HIP library")

    monkeypatch.setattr(E, "lib", no_lib)
    monkeypatch.setattr(S, "lib", no_lib)
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
    if cls == "SpectralFormer":
        assert m.pos_embedding.shape == (1, CASES[name][1]["C1"] + CASES[name][1]["C2"] + 1, 64)
        assert not hasattr(m, "conv2d")


def test_get_model_endnet_defaults():
    import vitcnn_amd
    from vitcnn_amd import AdamW, EndNet_Loss
    from vitcnn_amd.model_utils import REGISTERED, get_model
    assert "EndNet" in REGISTERED
    m, opt, crit, kw = get_model("EndNet", n_classes=16, n_bands=(144, 1), ignored_labels=[0], dataset="Houston2013",
                                 device=torch.device("cpu"))
    assert type(m) is vitcnn_amd.EndNet and type(opt) is AdamW and type(crit) is EndNet_Loss
    assert kw["patch_size"] == 1 and kw["applyPCA"] is False and kw["lr"] == 1e-3 and kw["epoch"] == 150
    assert kw["batch_size"] == 64 and kw["center_pixel"] is True and kw["supervision"] == "full"
    g = opt.param_groups[0]
    assert g["lr"] == 1e-3 and g["weight_decay"] == 0.0 and g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8
    assert float(crit.weight[0]) == 0.0 and float(crit.weight[1]) == 1.0
    assert m.encoder_fc1_a.weight.shape == (16, 144) and m.encoder_fc1_b.weight.shape == (16, 1)
    assert m.joint_encoder_fc7.weight.shape == (16, 64) and m.decoder_fc4_a.weight.shape == (144, 16)
    # applyPCA does not change n_bands for EndNet (model_utils.py:119-128)
    m2, _, _, kw2 = get_model("EndNet", n_classes=7, n_bands=(63, 2), ignored_labels=[0], dataset="x", applyPCA=True,
                              device=torch.device("cpu"))
    assert m2.C1 == 63 and m2.C2 == 2 and kw2["applyPCA"] is True


def test_get_model_spectralformer_defaults():
    import vitcnn_amd
    from vitcnn_amd import AdamW, CrossEntropyLoss
    from vitcnn_amd.model_utils import REGISTERED, get_model
    assert "SpectralFormer" in REGISTERED
    m, opt, crit, kw = get_model("SpectralFormer", n_classes=16, n_bands=(144, 1), ignored_labels=[0],
                                 dataset="Houston2013", device=torch.device("cpu"))
    assert type(m) is vitcnn_amd.SpectralFormer and type(opt) is AdamW and type(crit) is CrossEntropyLoss
    assert kw["patch_size"] == 1 and kw["applyPCA"] is False and kw["lr"] == 5e-4 and kw["epoch"] == 300
    assert kw["batch_size"] == 64 and kw["center_pixel"] is True and kw["supervision"] == "full"
    g = opt.param_groups[0]
    assert g["lr"] == 5e-4 and g["weight_decay"] == 0.0 and g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8
    assert float(crit.weight[0]) == 0.0 and float(crit.weight[1]) == 1.0
    assert m.pos_embedding.shape == (1, 146, 64) and m.patch_to_embedding.weight.shape == (64, 1)
    assert m.depth == 5 and m.heads == 4 and m.hidden == 8 and m.mode == "ViT" and m.p_drop == 0.1 and m.p_emb == 0.1
    assert m.mlp_head[1].weight.shape == (16, 64) and len(m.transformer.skipcat) == 3
    assert m.transformer.skipcat[0].weight.shape == (146, 146, 1, 2)
    # applyPCA: 30 HSI bands (model_utils.py:381-382)
    m2, _, _, kw2 = get_model("SpectralFormer", n_classes=7, n_bands=(63, 2), ignored_labels=[0], dataset="x",
                              applyPCA=True, device=torch.device("cpu"))
    assert m2.N == 32 and kw2["applyPCA"] is True


def test_endnet_constructor_accepts_and_rejects():
    from vitcnn_amd import EndNet
    for c1, c2, n in ((1, 1, 2), (145, 8, 64), (512, 512, 20)):
        EndNet(c1, c2, n)
    for c1, c2, n in ((0, 1, 16), (513, 1, 16), (30, 0, 16), (30, 513, 16), (30, 1, 1), (30, 1, 65)):
        with pytest.raises(ValueError):
            EndNet(c1, c2, n)


def test_spectralformer_constructor_accepts_and_rejects():
    from vitcnn_amd import SpectralFormer
    ok = dict(image_size=1, near_band=1, num_patches=31, num_classes=16, dim=64, depth=5, heads=4, mlp_dim=8)
    SpectralFormer(**ok)
    SpectralFormer(**dict(ok, num_patches=255))
    SpectralFormer(**dict(ok, num_patches=1))
    for bad in (dict(image_size=7), dict(near_band=3), dict(mode="CAF"), dict(dim_head=8), dict(num_patches=256),
                dict(num_patches=0)):
        with pytest.raises(ValueError):
            SpectralFormer(**dict(ok, **bad))


@pytest.mark.parametrize("name", ["endnet_b", "spectralformer_b"])
def test_pixel_cpu_input_raises(name):
    m = build(name)
    with pytest.raises(RuntimeError):
        m(torch.zeros(2, 13), torch.zeros(2, 2))
    with pytest.raises(RuntimeError):
        m(torch.zeros(2, 13, 1, 1), torch.zeros(2, 2, 1, 1))


def test_spectralformer_mask_raises():
    with pytest.raises(NotImplementedError):
        build("spectralformer_b")(torch.zeros(2, 13), torch.zeros(2, 2), mask=torch.ones(2, 15, dtype=torch.bool))


def test_endnet_train_mode_refuses_a_batch_of_one_and_more_than_the_bound():
    """torch's BatchNorm1d raises ValueError at B = 1 in training; so does this path, instead of returning NaN, and
    above the fused layer's bound (both before anything touches a device); eval at B = 1 goes on to the device check"""
    m = build("endnet_b").train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(torch.zeros(1, 13), torch.zeros(1, 2))
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(torch.zeros(1, 13, 1, 1), torch.zeros(1, 2, 1, 1))
    with pytest.raises(ValueError, match="at most 1024"):
        m(torch.zeros(1025, 13), torch.zeros(1025, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval()(torch.zeros(1, 13), torch.zeros(1, 2))


def test_endnet_loss_cpu_input_raises():
    from vitcnn_amd import EndNet_Loss
    o = torch.zeros(2, 4)
    with pytest.raises(RuntimeError):
        EndNet_Loss(weight=torch.ones(4))((o, o, o, o, o), torch.zeros(2, dtype=torch.int64))


def _raw():
    from vitcnn_amd._lib import lib
    return lib().raw


N = None
P16 = 16   # a never-dereferenced address
FWD_BN = (1, 1, 64, 16, 16, P16, 16, P16, P16, P16, P16, P16, P16, 1e-5, 0.1, P16, 16, P16, P16, P16, N)
BWD_BN = (1, 1, 64, 16, 16, P16, 16, P16, 16, P16, P16, 16, P16, P16, P16, 16, P16, P16, P16, P16, N)


def _with(args, **at):
    a = list(args)
    for i, v in at.items():
        a[int(i[1:])] = v
    return tuple(a)


REJECTED = [
    ("fc train B above the bound", "vc_fc_fused_fwd", _with(FWD_BN, a2=1025)),
    ("fc train B = 1", "vc_fc_fused_fwd", _with(FWD_BN, a2=1)),
    ("fc ldx < K", "vc_fc_fused_fwd", _with(FWD_BN, a6=15)),
    ("fc ldy < N", "vc_fc_fused_fwd", _with(FWD_BN, a16=15)),
    ("fc unknown mode", "vc_fc_fused_fwd", _with(FWD_BN, a0=3)),
    ("fc negative mode", "vc_fc_fused_fwd", _with(FWD_BN, a0=-1)),
    ("fc K = 513", "vc_fc_fused_fwd", _with(FWD_BN, a3=513, a6=513)),
    ("fc K = 0", "vc_fc_fused_fwd", _with(FWD_BN, a3=0)),
    ("fc train without xhat", "vc_fc_fused_fwd", _with(FWD_BN, a17=N)),
    ("fc BatchNorm without running statistics", "vc_fc_fused_fwd", _with(FWD_BN, a11=N)),
    ("fc without y", "vc_fc_fused_fwd", _with(FWD_BN, a15=N)),
    ("fc backward B above the bound", "vc_fc_fused_bwd", _with(BWD_BN, a2=1025)),
    ("fc backward ldx < K", "vc_fc_fused_bwd", _with(BWD_BN, a11=15)),
    ("fc backward lddy < N", "vc_fc_fused_bwd", _with(BWD_BN, a6=15)),
    ("fc backward ldy < N", "vc_fc_fused_bwd", _with(BWD_BN, a8=15)),
    ("fc backward lddz < N", "vc_fc_fused_bwd", _with(BWD_BN, a15=15)),
    ("fc backward unknown mode", "vc_fc_fused_bwd", _with(BWD_BN, a0=3)),
    ("fc backward BatchNorm without xhat", "vc_fc_fused_bwd", _with(BWD_BN, a9=N)),
    ("fc backward without dW", "vc_fc_fused_bwd", _with(BWD_BN, a16=N)),
    ("endnet loss B = 0", "vc_endnet_loss_fwd_bwd", (0, 16, 30, 1, P16, P16, N, P16, P16, P16, P16, P16, P16, P16, P16, N)),
    ("endnet loss C2 = 0", "vc_endnet_loss_fwd_bwd", (4, 16, 30, 0, P16, P16, N, P16, P16, P16, P16, P16, P16, P16, P16, N)),
    ("endnet loss without a gradient buffer", "vc_endnet_loss_fwd_bwd",
     (4, 16, 30, 1, P16, P16, N, P16, P16, P16, P16, P16, P16, N, P16, N)),
    ("embedding p = 1", "vc_sf_embed_fwd", (4, 30, 1, 64, P16, P16, P16, P16, P16, P16, 1.0, 0, P16, P16, N)),
    ("embedding dropout without a mask", "vc_sf_embed_fwd", (4, 30, 1, 64, P16, P16, P16, P16, P16, P16, 0.1, 0, P16, N, N)),
    ("embedding C1 = 0", "vc_sf_embed_fwd", (4, 0, 1, 64, P16, P16, P16, P16, P16, P16, 0.0, 0, P16, N, N)),
    ("embedding backward workspace too small", "vc_sf_embed_bwd",
     (4, 30, 1, 64, P16, P16, P16, N, 0.0, P16, P16, P16, P16, P16, 32 * 64 - 1, N)),
    ("embedding backward p < 0", "vc_sf_embed_bwd",
     (4, 30, 1, 64, P16, P16, P16, N, -0.5, P16, P16, P16, P16, P16, 32 * 64, N)),
]


@pytest.mark.parametrize("what,name,args", REJECTED, ids=[r[0] for r in REJECTED])
def test_pixel_host_side_rejections(what, name, args):
    """VC_REQUIRE returns 1 (hipErrorInvalidValue) before any launch: the pointers (null, or the never-dereferenced
    address 16) are not touched and no GPU is needed"""
    assert _raw()[name](*args) == 1, what
