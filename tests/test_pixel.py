"""EndNet and SpectralFormer on the MI355X: the HIP path (csrc/pixel.hip + S2EFT's encoder program, driven by
vitcnn_amd/endnet.py and vitcnn_amd/spectralformer.py) against the reference-generated fixtures
(tests/golden/endnet_*.npz, spectralformer_*.npz), at B = 64 on the Houston2013 shape against the float64 restatement
tests/pixel_oracle.py (which tests/test_pixel_cpu.py pins to the same fixtures), and end to end at patch_size 1
through PatchBatcher, train() and test().

Rules: outputs, loss and eval outputs within 1e-3 relative with the same argmax (the project's parity rule); running
statistics rtol 1e-3 / atol 1e-4 and num_batches_tracked exact (test_mdlrs.py's rule); every parameter gradient within
1e-3 of its norm + 1e-5 of the step's largest gradient norm (test_s2eft.py / test_mft.py; the absolute term covers the
Linear biases in front of a train-mode BatchNorm, whose true gradient is 0).
"""
import functools

import numpy as np
import pytest
import torch

import pixel_oracle as O
from pixel_cases import CASES, N_KEYS, build, golden, spectralformer

pytestmark = pytest.mark.gpu

UNUSED = {"EndNet": "joint_encoder_bn7.", "SpectralFormer": "transformer.skipcat."}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _rel(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))


def _criterion(cls, w):
    from vitcnn_amd.losses import CrossEntropyLoss, EndNet_Loss
    return (EndNet_Loss if cls == "EndNet" else CrossEntropyLoss)(weight=w.cuda())


def _flat_grads(m):
    flat = m.flat_params.grad
    named = dict(m.named_parameters())
    return {n: flat[o:o + named[n].numel()].view(named[n].shape).cpu() for n, o in m._poff.items()}


def _outs(cls, out):
    return tuple(o.detach().cpu() for o in (out[:3] if cls == "EndNet" else (out,)))


def _step(m, cls, x1, x2, t, w):
    out = m(x1.cuda(), x2.cuda())
    loss = _criterion(cls, w)(out, t.cuda())
    loss.backward()
    torch.cuda.synchronize()
    return out, _outs(cls, out), float(loss.detach()), _flat_grads(m)


def _check_outs_loss(tag, got_all, hloss, ref_all, ref_loss):
    assert len(got_all) == len(ref_all)
    for i, (got, ref) in enumerate(zip(got_all, ref_all)):
        print(f"{tag}: output {i} rel {_rel(got, ref):.3e}")
        assert got.shape == ref.shape and torch.isfinite(got).all()
        assert _rel(got, ref) < 1e-3, (i, _rel(got, ref))
    assert torch.equal(got_all[0].argmax(1), ref_all[0].argmax(1))
    if ref_loss is not None:
        print(f"{tag}: loss rel {abs(hloss - ref_loss) / abs(ref_loss):.3e}")
        assert abs(hloss - ref_loss) <= 1e-3 * abs(ref_loss)


def _check_grads(tag, hg, ref_grads):
    gmax = max(float(g.double().norm()) for g in ref_grads.values())
    worst = ("", 0.0)
    assert set(hg) == set(ref_grads)
    for k, g in ref_grads.items():
        err = float((hg[k].double() - g.double()).norm())
        bound = 1e-3 * float(g.double().norm()) + 1e-5 * gmax
        worst = max(worst, (k, err / bound), key=lambda r: r[1])
        assert err <= bound, (k, err, float(g.double().norm()), gmax)
    print(f"{tag}: worst gradient {worst[0]} at {worst[1]:.3f} of the rule (gmax {gmax:.3e})")


def _check_running(m, ref_running):
    bufs = dict(m.named_buffers())
    assert set(ref_running) == set(bufs)
    for k, v in ref_running.items():
        if k.endswith("num_batches_tracked"):
            assert int(bufs[k]) == int(v), k
        else:
            assert torch.allclose(bufs[k].cpu(), v.float(), rtol=1e-3, atol=1e-4), k


def _check_unused_stay_put_under_a_step(m, cls, sd, lr):
    """one fused optimizer step on the gradient just computed: the parameters the forward never applies (zero
    gradient) keep their bits, every other parameter tensor moves; the unused BatchNorm's buffers stay initial"""
    from vitcnn_amd.optim import AdamW
    pfx = UNUSED[cls]
    flat = _flat_grads(m)
    unused = [k for k in flat if k.startswith(pfx)]
    assert len(unused) == (2 if cls == "EndNet" else 6)
    assert not any(flat[k].any() for k in unused)
    opt = AdamW(m.parameters(), lr=lr, weight_decay=0.0)
    opt.step()
    torch.cuda.synchronize()
    after = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    for k in sd:
        if k.startswith(pfx):
            assert torch.equal(after[k], sd[k]), k
    moved = [k for k in flat if not k.startswith(pfx) and not torch.equal(after[k], sd[k])]
    assert len(moved) >= 0.9 * (len(flat) - len(unused)), (len(moved), len(flat))


@pytest.mark.parametrize("name", list(CASES))
def test_pixel_gpu_golden(name):
    _need_gpu()
    cls, case = CASES[name]
    sd, run, gr, t = golden(name)
    m = build(name)
    m.load_state_dict(sd)
    m = m.to("cuda").train()
    out, ho, hloss, hg = _step(m, cls, t["x1"], t["x2"], t["target"], t["weight"])
    assert ho[0].shape == (case["B"], case["ncls"])
    if cls == "EndNet":
        # the 5-tuple: the last two elements are the inputs as [B, C]
        assert len(out) == 5 and torch.equal(out[3].cpu(), t["x1"]) and torch.equal(out[4].cpu(), t["x2"])
    _check_outs_loss(name, ho, hloss, t["outs"], t["loss"])
    _check_grads(name, hg, gr)
    _check_running(m, run)
    m.eval()
    with torch.no_grad():
        ev = m(t["x1"].cuda().view(case["B"], case["C1"], 1, 1), t["x2"].cuda().view(case["B"], case["C2"], 1, 1))
    assert (len(ev) == 5) if cls == "EndNet" else torch.is_tensor(ev)
    _check_outs_loss(name + " eval", _outs(cls, ev), None, t["eval_outs"], None)
    _check_running(m, run)            # an eval forward moves no statistic and no counter
    m.train()
    _check_unused_stay_put_under_a_step(m, cls, dict(sd, **run), 1e-3)


@functools.lru_cache(maxsize=None)
def _b64_inputs():
    g = torch.Generator().manual_seed(1)
    x1, x2 = torch.rand(64, 144, generator=g), torch.rand(64, 1, generator=g)
    t = torch.randint(1, 16, (64,), generator=g)
    w = torch.ones(16)
    w[0] = 0
    return x1, x2, t, w


def test_endnet_gpu_b64_houston_shape_against_the_oracle():
    """B 64, 144 + 1 bands, 16 classes, seed 1 inputs: in float64 every BatchNorm output in front of a ReLU keeps 1e-5
    from 0 (asserted), so no element is excluded and every gradient is held to the rule"""
    _need_gpu()
    from vitcnn_amd import EndNet
    torch.manual_seed(0)
    m = EndNet(144, 1, 16)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x1, x2, t, w = _b64_inputs()
    outs, loss, grads, running, pre = O.endnet_train_step(sd, x1, x2, t, w)
    margin = min(float(v.abs().min()) for v in pre.values())
    print(f"EndNet b64: smallest |BatchNorm output| in float64 {margin:.3e}")
    assert len(pre) == 10 and margin >= 1e-5
    m = m.to("cuda").train()
    _, ho, hloss, hg = _step(m, "EndNet", x1, x2, t, w)
    _check_outs_loss("EndNet b64", ho, hloss, outs, float(loss))
    _check_grads("EndNet b64", hg, grads)
    _check_running(m, running)
    m.eval()
    with torch.no_grad():
        ev = m(x1.cuda(), x2.cuda())
    _check_outs_loss("EndNet b64 eval", _outs("EndNet", ev), None, O.endnet_eval(dict(sd, **running), x1, x2), None)


def test_spectralformer_gpu_b64_with_dropout_against_the_oracle_with_the_same_masks():
    """get_model's configuration (dropout 0.1 at the embedding and the three sites of each layer): keep fraction ~0.9,
    and logits, loss and every gradient equal the oracle's evaluated with the HIP path's own keep masks"""
    _need_gpu()
    from helpers import cpu_masks, program_spy
    torch.manual_seed(0)
    m = spectralformer(145, 16, dropout=0.1)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x1, x2, t, w = _b64_inputs()
    m = m.to("cuda").train()
    with program_spy(type(m)) as progs:
        _, ho, hloss, hg = _step(m, "SpectralFormer", x1, x2, t, w)
    masks = cpu_masks(progs[-1])
    assert set(masks) == {"emb"} | {f"{i}.{s}" for i in range(5) for s in ("attn", "ff1", "ff2")}
    assert masks["emb"].numel() == 64 * 146 * 64
    keep = torch.cat(list(masks.values())).mean().item()
    assert 0.89 < keep < 0.91, keep
    logits, loss, grads = O.sf_train_step(sd, x1, x2, t, w, drop={k: (v, 0.1) for k, v in masks.items()})
    _check_outs_loss("SpectralFormer b64 p=0.1", ho, hloss, (logits,), float(loss))
    _check_grads("SpectralFormer b64 p=0.1", hg, grads)
    m.eval()
    with torch.no_grad():
        ev = m(x1.cuda(), x2.cuda())
    _check_outs_loss("SpectralFormer b64 eval", (ev.cpu(),), None, (O.sf_eval(sd, x1, x2),), None)   # eval: no dropout


@pytest.mark.parametrize("cls", ["EndNet", "SpectralFormer"])
def test_pixel_backward_repeats_its_bits(cls):
    """the autograd.Function forward plus .backward(): two identical calls (SpectralFormer with dropout 0.1 and the
    same torch seed, i.e. the same masks) give the same flat gradient bits -- every sum runs in a fixed order"""
    _need_gpu()
    from vitcnn_amd import EndNet
    torch.manual_seed(0)
    m = (EndNet(144, 1, 16) if cls == "EndNet" else spectralformer(145, 16, dropout=0.1)).to("cuda").train()
    x1, x2, t, w = _b64_inputs()
    got = []
    for _ in range(2):
        m.zero_grad()
        torch.manual_seed(123)
        _, ho, hloss, _ = _step(m, cls, x1, x2, t, w)
        got.append((ho, hloss, m.flat_params.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(got[0][0], got[1][0])) and got[0][1] == got[1][1]
    assert torch.equal(got[0][2], got[1][2]) and float(got[0][2].norm()) > 0


def test_endnet_loss_scales_its_saved_gradients_by_the_incoming_gradient():
    _need_gpu()
    from vitcnn_amd import EndNet_Loss
    g = torch.Generator().manual_seed(3)
    out, de1, de2 = (torch.rand(5, n, generator=g).cuda().requires_grad_(True) for n in (12, 13, 2))
    x1, x2 = torch.rand(5, 13, 1, 1, generator=g).cuda(), torch.rand(5, 2, generator=g).cuda()
    t = torch.randint(1, 12, (5,), generator=g).cuda()
    w = torch.ones(12)
    w[0] = 0
    crit = EndNet_Loss(weight=w).cuda()
    (3.0 * crit((out, de1, de2, x1, x2), t)).backward()
    ref = [v.detach().double().cpu().requires_grad_(True) for v in (out, de1, de2)]
    (3.0 * O.endnet_loss(*ref, x1.double().cpu(), x2.double().cpu(), t.cpu(), w.double())).backward()
    for a, b in zip((out, de1, de2), ref):
        assert _rel(a.grad.cpu(), b.grad) < 1e-5


# ---------------------------------------------------------------------------------------------- patch_size 1, end to end
SCENE_W, SCENE_H, SCENE_C1, SCENE_C2, SCENE_CLS = 12, 10, 13, 2, 4


@functools.lru_cache(maxsize=None)
def _scene():
    """a 12 x 10 scene of three classes in blocks (label 0 = unlabelled at a few pixels), each with its own spectrum +
    noise"""
    g = torch.Generator().manual_seed(11)
    xs, ys = torch.meshgrid(torch.arange(SCENE_W), torch.arange(SCENE_H), indexing="ij")
    gt = 1 + ((xs // 4 + ys // 5) % 3)
    gt[torch.rand(SCENE_W, SCENE_H, generator=g) < 0.15] = 0
    proto = torch.rand(SCENE_CLS, SCENE_C1 + SCENE_C2, generator=g)
    cube = proto[1 + ((xs // 4 + ys // 5) % 3)] + 0.05 * torch.randn(SCENE_W, SCENE_H, SCENE_C1 + SCENE_C2, generator=g)
    return cube[:, :, :SCENE_C1].numpy().copy(), cube[:, :, SCENE_C1:].numpy().copy(), gt.numpy().astype(np.int64)


def test_patch_batcher_at_patch_size_1_yields_the_labelled_pixels_spectra():
    _need_gpu()
    from vitcnn_amd.window import PatchBatcher
    img1, img2, gt = _scene()
    loader = PatchBatcher(img1, img2, gt, 1, ignored_labels=(0,), batch_size=16, device="cuda", seed=0)
    inner = gt[1:, 1:]                  # the reference keeps centres with x > p and y > p (datasets.py:497), p = 0
    assert len(loader.centers) == int((inner != 0).sum()) and len(loader) == -(-len(loader.centers) // 16)
    seen = 0
    for x1, x2, t in loader:
        n = x1.shape[0]
        assert x1.shape == (n, SCENE_C1, 1, 1) and x2.shape == (n, SCENE_C2, 1, 1) and t.shape == (n,)
        c = loader.centers[seen:seen + n]
        assert np.array_equal(x1.cpu().numpy()[:, :, 0, 0], img1[c[:, 0], c[:, 1]])
        assert np.array_equal(x2.cpu().numpy()[:, :, 0, 0], img2[c[:, 0], c[:, 1]])
        assert np.array_equal(t.cpu().numpy(), gt[c[:, 0], c[:, 1]]) and (t != 0).all()
        seen += n
    assert seen == len(loader.centers)


@pytest.mark.parametrize("cls", ["EndNet", "SpectralFormer"])
def test_pixel_train_and_test_plugin_surface(cls, tmp_path, monkeypatch):
    """two epochs of train() over a PatchBatcher at patch_size 1 (the eager TrainStepper path) give finite losses and
    changed parameters and report the launch mode; test() returns [W, H, n_classes] equal to the model's own eval
    forward over all pixels"""
    _need_gpu()
    from vitcnn_amd import model_utils as mu
    from vitcnn_amd.window import PatchBatcher, window_count
    monkeypatch.chdir(tmp_path)
    img1, img2, gt = _scene()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m, opt, crit, kw = mu.get_model(cls, n_classes=SCENE_CLS, n_bands=(SCENE_C1, SCENE_C2), ignored_labels=[0],
                                    dataset="synthetic", device=dev)
    assert kw["patch_size"] == 1
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    loader = PatchBatcher(img1, img2, gt, 1, ignored_labels=(0,), batch_size=16, device=dev, seed=0)
    nb = len(loader)
    assert nb >= 4 and len(loader.centers) % 16 != 1      # train-mode BatchNorm1d needs two rows (as in torch)
    mu.train("t", 0, None, m, opt, crit, loader, 2, device=dev, display_iter=0)
    st = mu.train.last_stats
    assert st["launch"] == "eager" and len(st["losses"]) == 2 * nb
    print(f"{cls}: mean loss of epoch 1 {np.mean(st['losses'][:nb]):.4f}, of epoch 2 {np.mean(st['losses'][nb:]):.4f}")
    assert np.isfinite(st["losses"]).all()
    pfx = UNUSED[cls]
    for k, v in m.named_parameters():
        assert torch.isfinite(v).all()
        assert torch.equal(v, before[k]) == k.startswith(pfx), k
    ck = [p for p in (tmp_path / "checkpoints").rglob("*.pth") if "final_epoch" in str(p)]
    assert ck and len(torch.load(ck[0], map_location="cpu")) == N_KEYS[cls]
    # whole-image inference: every pixel is a window
    n = window_count(SCENE_W, SCENE_H, 1, 1)
    assert n == SCENE_W * SCENE_H
    probs = mu.test(0, m, img1, img2, dict(kw, n_classes=SCENE_CLS, batch_size=64, test_stride=1))
    assert probs.shape == (SCENE_W, SCENE_H, SCENE_CLS) and probs.dtype == np.float64
    m.eval()
    with torch.no_grad():
        out = m(torch.from_numpy(img1).reshape(n, SCENE_C1).cuda(), torch.from_numpy(img2).reshape(n, SCENE_C2).cuda())
    out = (out[0] if cls == "EndNet" else out).cpu()
    assert out.shape == (n, SCENE_CLS)
    assert _rel(torch.from_numpy(probs.reshape(n, SCENE_CLS)).float(), out) < 1e-5
