"""MFT comparison model: the float64 restatement pinned to the reference, the HIP path against both.

CPU tests: tests/mft_oracle.py reproduces the reference module's own train logits, loss, every parameter
gradient, BatchNorm running statistics and eval logits (tests/golden/mft_b4.npz, mft_odd_b4.npz and their
_grads.npz, made by tests/golden/gen_mft_golden.py from the reference's MFT.py); the product module constructs
without the HIP library and has the reference's state_dict names, shapes and, seeded alike, initial values.
GPU tests: the HIP path (csrc/mft.hip + the conv / norm / GEMM entry points) against the fixtures (B = 4, both
HetConv group counts) and against the oracle at B = 64 (30 and 144 bands): logits and loss within 1e-3 relative,
argmax identical, every parameter gradient within 1e-3 of its norm + 1e-5 of the step's largest gradient norm
(the rule of test_s2eft.py / test_fusatnet.py; it also bounds the four conv biases whose true gradient is zero
because a train-mode BatchNorm follows them), running statistics and eval logits; dropout with the HIP path's
own keep masks fed to the oracle; vitcnn_amd.optim.Adam against torch.optim.Adam; train() and test().
"""
import functools
import os

import numpy as np
import pytest
import torch

import mft_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
KW = {"mft_b4": dict(patch_size=11, FM=16, NC=30, NCLidar=1, Classes=16, HSIOnly=False),
      "mft_odd_b4": dict(patch_size=7, FM=16, NC=11, NCLidar=2, Classes=12, HSIOnly=False)}
ZERO_GRAD_BIASES = ("conv5.0.bias", "conv6.0.gwc.bias", "conv6.0.pwc.bias", "lidarConv.0.bias")


@functools.lru_cache(maxsize=None)
def _golden(name):
    z = np.load(os.path.join(HERE, "golden", name + ".npz"))
    zg = np.load(os.path.join(HERE, "golden", name + "_grads.npz"))
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p:")}
    run = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("r:")}
    gr = {k[2:]: torch.from_numpy(zg[k]) for k in zg.files}
    t = {k: torch.from_numpy(z[k]) for k in ("x1", "x2", "target", "weight", "logits", "eval_logits")}
    t["loss"] = float(z["loss"])
    return sd, run, gr, t


def _rel(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))


# ---------------------------------------------------------------- CPU
@pytest.mark.parametrize("name", list(KW))
def test_mft_oracle_matches_reference(name):
    sd, run, gr, t = _golden(name)
    logits, loss, grads, running, _ = O.train_step(sd, t["x1"], t["x2"], t["target"], t["weight"])
    assert torch.allclose(logits.float(), t["logits"], rtol=1e-5, atol=1e-5)
    assert abs(float(loss) - t["loss"]) <= 1e-5 + 1e-5 * abs(t["loss"])
    assert set(grads) == set(gr) and len(sd) == 58
    for k, g in gr.items():
        assert torch.allclose(grads[k].float(), g, rtol=1e-4, atol=1e-6), (k, float((grads[k].float() - g).abs().max()))
    for k, v in running.items():
        assert torch.allclose(v.float(), run[k], rtol=1e-5, atol=1e-6), k
    after = dict(sd, **run)
    assert torch.allclose(O.eval_logits(after, t["x1"], t["x2"]).float(), t["eval_logits"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", list(KW))
def test_mft_constructs_without_the_library_with_the_reference_state_dict(name, monkeypatch):
    import vitcnn_amd.mft as M

    def no_lib():
        raise AssertionError("constructing MFT must not load the HIP library")

    monkeypatch.setattr(M, "lib", no_lib)
    sd, _, gr, _ = _golden(name)
    torch.manual_seed(0)
    m = M.MFT(**KW[name])
    mine = m.state_dict()
    assert list(mine.keys()) == list(sd.keys()) and len(mine) == 58
    for k in sd:
        assert mine[k].shape == sd[k].shape, k
        assert torch.equal(mine[k], sd[k]), k   # same creation order and initialisers -> the same draws
    assert [n for n, _ in m.named_parameters()] == list(gr.keys())
    assert m.HSIOnly is False


def test_mft_constructor_rejects_unsupported_shapes():
    from vitcnn_amd.mft import MFT
    for bad in (dict(NC=8), dict(NC=4097), dict(FM=8), dict(patch_size=4), dict(patch_size=29), dict(NCLidar=0)):
        with pytest.raises(ValueError):
            MFT(**dict(KW["mft_b4"], **bad))


def test_get_model_mft_defaults():
    from vitcnn_amd import MFT, Adam, CrossEntropyLoss
    from vitcnn_amd.model_utils import REGISTERED, get_model
    assert "MFT" in REGISTERED
    m, opt, crit, kw = get_model("MFT", n_classes=16, n_bands=(144, 1), ignored_labels=[0], dataset="Houston2013",
                                 device=torch.device("cpu"))
    assert type(m) is MFT and type(opt) is Adam and type(crit) is CrossEntropyLoss
    assert kw["patch_size"] == 11 and kw["applyPCA"] is False and kw["lr"] == 5e-4 and kw["epoch"] == 500
    assert kw["batch_size"] == 64 and kw["center_pixel"] is True and kw["supervision"] == "full"
    g = opt.param_groups[0]
    assert g["lr"] == 5e-4 and g["weight_decay"] == 5e-3 and g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8
    assert m.NC == 144 and m.NCLidar == 1 and m.patchsize == 11 and m.groups == 16
    assert m.conv6[0].gwc.weight.shape == (64, 68, 3, 3) and m.out3.weight.shape == (16, 64)
    assert float(crit.weight[0]) == 0.0 and float(crit.weight[1]) == 1.0
    m2, _, _, kw2 = get_model("MFT", n_classes=7, n_bands=(63, 2), ignored_labels=[0], dataset="x", applyPCA=True,
                              device=torch.device("cpu"))
    assert m2.NC == 30 and m2.NCLidar == 2 and kw2["applyPCA"] is True


def test_mft_cpu_input_raises():
    from vitcnn_amd.mft import MFT
    m = MFT(**KW["mft_odd_b4"])
    with pytest.raises(RuntimeError):
        m(torch.zeros(2, 11, 7, 7), torch.zeros(2, 2, 7, 7))


# ---------------------------------------------------------------- GPU parity
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _model(kw, sd, p_drop=0.0):
    from vitcnn_amd.mft import MFT
    m = MFT(**kw)
    m.load_state_dict(sd)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = p_drop
    return m.to("cuda").train()


def _flat_grads(m):
    flat = m.flat_params.grad
    named = dict(m.named_parameters())
    return {n: flat[o:o + named[n].numel()].view(named[n].shape).cpu() for n, o in m._poff.items()}


def _step(m, x1, x2, t, w):
    from vitcnn_amd.losses import CrossEntropyLoss
    logits = m(x1.cuda(), x2.cuda())
    loss = CrossEntropyLoss(weight=w.cuda())(logits, t.cuda())
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach().cpu(), float(loss.detach()), _flat_grads(m)


def _check_step(tag, got, ref_logits, ref_loss, ref_grads):
    hl, hloss, hg = got
    print(f"MFT {tag}: logits rel {_rel(hl, ref_logits):.3e}, loss rel {abs(hloss - ref_loss) / abs(ref_loss):.3e}")
    assert torch.isfinite(hl).all()
    assert _rel(hl, ref_logits) < 1e-3, _rel(hl, ref_logits)
    assert torch.equal(hl.argmax(1), ref_logits.argmax(1))
    assert abs(hloss - ref_loss) <= 1e-3 * abs(ref_loss)
    gmax = max(float(g.double().norm()) for g in ref_grads.values())
    worst = ("", 0.0)
    for k, g in ref_grads.items():
        err = float((hg[k].double() - g.double()).norm())
        bound = 1e-3 * float(g.double().norm()) + 1e-5 * gmax
        worst = max(worst, (k, err / bound), key=lambda r: r[1])
        assert err <= bound, (k, err, float(g.double().norm()), gmax)
    print(f"MFT {tag}: worst gradient {worst[0]} at {worst[1]:.3f} of the rule (gmax {gmax:.3e})")
    assert set(ZERO_GRAD_BIASES) <= set(hg)


def _check_after(m, x1, x2, ref_running, ref_eval):
    bufs = dict(m.named_buffers())
    for k, v in ref_running.items():
        if k.endswith("num_batches_tracked"):
            assert int(bufs[k]) == int(v), k
        else:
            assert torch.allclose(bufs[k].cpu(), v.float(), rtol=1e-3, atol=1e-4), k
    m.eval()
    with torch.no_grad():
        le = m(x1.cuda(), x2.cuda()).cpu()
    assert _rel(le, ref_eval) < 1e-3, _rel(le, ref_eval)
    m.train()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(KW))
def test_mft_gpu_golden(name):
    _need_gpu()
    sd, run, gr, t = _golden(name)
    m = _model(KW[name], sd)
    got = _step(m, t["x1"], t["x2"], t["target"], t["weight"])
    _check_step(name, got, t["logits"], t["loss"], gr)
    _check_after(m, t["x1"], t["x2"], run, t["eval_logits"])


@functools.lru_cache(maxsize=None)
def _b64_case(NC):
    """B = 64 at patch 11, 16 classes: seeded initial state, inputs, and the float64 oracle's step"""
    from vitcnn_amd.mft import MFT
    kw = dict(KW["mft_b4"], NC=NC)
    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in MFT(**kw).state_dict().items()}
    g = torch.Generator().manual_seed(5)
    x1, x2 = torch.rand(64, NC, 11, 11, generator=g), torch.rand(64, 1, 11, 11, generator=g)
    t = torch.randint(1, 16, (64,), generator=g)
    w = torch.ones(16)
    w[0] = 0
    logits, loss, grads, running, pre = O.train_step(sd, x1, x2, t, w)
    after = dict(sd, **running)
    return kw, sd, x1, x2, t, w, logits, float(loss), grads, running, O.eval_logits(after, x1, x2)


@pytest.mark.gpu
@pytest.mark.parametrize("NC", [30, 144])
def test_mft_gpu_b64_against_the_oracle(NC):
    _need_gpu()
    kw, sd, x1, x2, t, w, logits, loss, grads, running, ev = _b64_case(NC)
    m = _model(kw, sd)
    _check_step(f"b64 NC={NC}", _step(m, x1, x2, t, w), logits, loss, grads)
    _check_after(m, x1, x2, running, ev)


@pytest.mark.gpu
def test_mft_gpu_dropout_train():
    """dropout 0.1 at the reference's five sites: keep fraction ~0.9, logits and every gradient equal the oracle's
    evaluated with the HIP path's own keep masks; eval afterwards applies none"""
    _need_gpu()
    from helpers import cpu_masks, program_spy
    sd, run, _, t = _golden("mft_b4")
    m = _model(KW["mft_b4"], sd, p_drop=0.1)
    with program_spy(type(m)) as progs:
        got = _step(m, t["x1"], t["x2"], t["target"], t["weight"])
    masks = cpu_masks(progs[-1])
    assert set(masks) == {"emb"} | {f"{i}.{s}" for i in range(2) for s in ("attn", "ff1", "ff2")}
    keep = torch.cat(list(masks.values())).mean().item()
    assert 0.88 < keep < 0.92, keep
    drop = {k: (v, 0.1) for k, v in masks.items()}
    logits, loss, grads, running, _ = O.train_step(sd, t["x1"], t["x2"], t["target"], t["weight"], drop=drop)
    _check_step("dropout", got, logits, float(loss), grads)
    assert _rel(logits.float(), t["logits"]) > 1e-3   # the masks did something
    _check_after(m, t["x1"], t["x2"], run, t["eval_logits"])   # eval: the no-dropout forward


@pytest.mark.gpu
def test_mft_adam_matches_torch_adam_and_gradients_repeat():
    """get_model('MFT')'s optimizer (vc_adam over the flat buffer: coupled L2) against torch.optim.Adam(lr 5e-4,
    weight_decay 5e-3) fed the same gradients, 3 steps; a second run of the same step gives the same bits"""
    _need_gpu()
    from vitcnn_amd.optim import Adam
    sd, _, _, t = _golden("mft_odd_b4")
    m = _model(KW["mft_odd_b4"], sd)
    ref = {k: v.detach().clone() for k, v in m.named_parameters()}
    ref_params = [torch.nn.Parameter(v) for v in ref.values()]
    topt = torch.optim.Adam(ref_params, lr=5e-4, weight_decay=5e-3)
    opt = Adam(m.parameters(), lr=5e-4, weight_decay=5e-3)
    for it in range(3):
        opt.zero_grad()
        _step(m, t["x1"], t["x2"], t["target"], t["weight"])
        g1 = m.flat_params.grad.clone()
        if it == 0:
            opt.zero_grad()
            _step(m, t["x1"], t["x2"], t["target"], t["weight"])
            assert torch.equal(m.flat_params.grad, g1)
        grads = _flat_grads(m)
        for p, k in zip(ref_params, ref):
            p.grad = grads[k].cuda().clone()
        opt.step()
        topt.step()
        torch.cuda.synchronize()
    named = dict(m.named_parameters())
    moved = 0.0
    for p, k in zip(ref_params, ref):
        assert torch.allclose(named[k].detach(), p.detach(), rtol=1e-5, atol=1e-6), k
        moved = max(moved, float((p.detach() - sd[k].cuda()).abs().max()))
    assert moved > 1e-4


class _Loader(list):
    class _DS:
        name = "synthetic"
        ignored_labels = [0]

    dataset = _DS()


@pytest.mark.gpu
def test_mft_train_and_test_plugin_surface(tmp_path, monkeypatch):
    """two epochs of train() over a tiny in-memory loader (the eager TrainStepper path) reduce the loss and write a
    checkpoint with the reference's key set; test() over a 16 x 16 scene matches the batched eval logits by argmax"""
    _need_gpu()
    from vitcnn_amd import model_utils as mu
    monkeypatch.chdir(tmp_path)
    sd, _, _, t = _golden("mft_odd_b4")
    torch.manual_seed(0)
    m, opt, crit, kw = mu.get_model("MFT", n_classes=12, n_bands=(11, 2), ignored_labels=[0], dataset="synthetic",
                                    patch_size=7, device=torch.device("cuda"))
    m.load_state_dict(sd)
    for mod in m.modules():   # the same two batches every epoch: without dropout the loss must fall
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    x1, x2, tg = t["x1"].cuda(), t["x2"].cuda(), t["target"].cuda()
    loader = _Loader([(x1, x2, tg), (x1.flip(0), x2.flip(0), tg.flip(0))])
    mu.train("t", 0, None, m, opt, crit, loader, 2, device=torch.device("cuda"), display_iter=0)
    st = mu.train.last_stats
    assert st["launch"] == "eager" and len(st["losses"]) == 4
    assert st["losses"][-1] < st["losses"][0], st["losses"]
    ck = [p for p in (tmp_path / "checkpoints").rglob("*.pth") if "final_epoch" in str(p)]
    assert ck
    loaded = torch.load(ck[0], map_location="cpu")
    assert list(loaded.keys()) == list(sd.keys())
    assert all(loaded[k].shape == sd[k].shape for k in sd)
    # whole-image inference
    g = torch.Generator().manual_seed(3)
    img1, img2 = torch.rand(16, 16, 11, generator=g).numpy(), torch.rand(16, 16, 2, generator=g).numpy()
    hp = dict(kw, n_classes=12, batch_size=8, test_stride=1)
    probs = mu.test(0, m, img1, img2, hp)
    assert probs.shape == (16, 16, 12)
    xs = [(x, y) for x in range(10) for y in range(10)]
    b1 = torch.stack([torch.from_numpy(img1[x:x + 7, y:y + 7]).permute(2, 0, 1) for x, y in xs])
    b2 = torch.stack([torch.from_numpy(img2[x:x + 7, y:y + 7]).permute(2, 0, 1) for x, y in xs])
    m.eval()
    with torch.no_grad():
        ref = m(b1.cuda(), b2.cuda()).cpu()
    got = torch.from_numpy(np.stack([probs[x + 3, y + 3] for x, y in xs]))
    assert torch.equal(got.argmax(1), ref.argmax(1))
    assert _rel(got.float(), ref) < 1e-5
