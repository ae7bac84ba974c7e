"""MDL-RS fusion CNNs on the MI355X: the HIP path (csrc/mdlrs.hip + the conv / norm / GEMM entry points, driven by
vitcnn_amd/mdlrs.py) against the reference-generated fixtures (tests/golden/mdlrs_*.npz) and, at B = 64 on the
Houston2013 shape, against the float64 restatement tests/mdlrs_oracle.py (which tests/test_mdlrs_cpu.py pins to the
same fixtures).

Rules: logits, loss and eval logits within 1e-3 relative (the project's parity rule); running statistics rtol 1e-3 /
atol 1e-4 and num_batches_tracked exact (test_mft.py's rule -- the counters and the non-commutative running averages
are what a wrong application order of Cross_fusion_CNN's shared BatchNorms would break); every parameter gradient
within 1e-3 of its norm + 1e-5 of the step's largest gradient norm (the absolute term covers the conv biases in
front of a train-mode BatchNorm, whose true gradient is 0).  The B = 64 test checks logits and loss only: a ReLU or
pool decision flipped at a near-tie moves them continuously, but not the gradients.
"""
import functools

import numpy as np
import pytest
import torch

import mdlrs_oracle as O
from mdlrs_cases import CASES, N_KEYS, build, golden

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _rel(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))


def _tup(out):
    return out if isinstance(out, tuple) else (out,)


def _criterion(cls, w):
    from vitcnn_amd.losses import Cross_fusion_CNN_Loss, CrossEntropyLoss
    return (Cross_fusion_CNN_Loss if cls == "Cross_fusion_CNN" else CrossEntropyLoss)(weight=w.cuda())


def _flat_grads(m):
    flat = m.flat_params.grad
    named = dict(m.named_parameters())
    return {n: flat[o:o + named[n].numel()].view(named[n].shape).cpu() for n, o in m._poff.items()}


def _step(m, cls, x1, x2, t, w):
    out = m(x1.cuda(), x2.cuda())
    loss = _criterion(cls, w)(out, t.cuda())
    loss.backward()
    torch.cuda.synchronize()
    return tuple(o.detach().cpu() for o in _tup(out)), float(loss.detach()), _flat_grads(m)


def _check_logits_loss(tag, hl, hloss, ref_logits, ref_loss):
    assert len(hl) == len(ref_logits)
    for i, (got, ref) in enumerate(zip(hl, ref_logits)):
        print(f"{tag}: logits{i + 1} rel {_rel(got, ref):.3e}")
        assert got.shape == ref.shape and torch.isfinite(got).all()
        assert _rel(got, ref) < 1e-3, (i, _rel(got, ref))
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


def _check_after(m, x1, x2, ref_running, ref_eval):
    bufs = dict(m.named_buffers())
    assert set(ref_running) == set(bufs)
    for k, v in ref_running.items():
        if k.endswith("num_batches_tracked"):
            assert int(bufs[k]) == int(v), k
        else:
            assert torch.allclose(bufs[k].cpu(), v.float(), rtol=1e-3, atol=1e-4), k
    m.eval()
    with torch.no_grad():
        le = _tup(m(x1.cuda(), x2.cuda()))
    assert len(le) == len(ref_eval)
    for got, ref in zip(le, ref_eval):
        assert _rel(got.cpu(), ref) < 1e-3, _rel(got.cpu(), ref)
    m.train()


@pytest.mark.parametrize("name", list(CASES))
def test_mdlrs_gpu_golden(name):
    _need_gpu()
    cls, case = CASES[name]
    sd, run, gr, t = golden(name)
    m = build(name)
    m.load_state_dict(sd)
    m = m.to("cuda").train()
    hl, hloss, hg = _step(m, cls, t["x1"], t["x2"], t["target"], t["weight"])
    assert all(o.shape == (case["B"], case["ncls"]) for o in hl)
    _check_logits_loss(name, hl, hloss, t["logits"], t["loss"])
    _check_grads(name, hg, gr)
    _check_after(m, t["x1"], t["x2"], run, t["eval_logits"])


@functools.lru_cache(maxsize=None)
def _b64_case(cls):
    """B = 64 on the Houston2013 shape (144 + 1 bands, patch 7, 16 classes): seeded initial state and inputs, and
    the float64 oracle's logits and loss"""
    from vitcnn_amd import mdlrs
    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in getattr(mdlrs, cls)(144, 1, 16).state_dict().items()}
    g = torch.Generator().manual_seed(5)
    x1, x2 = torch.rand(64, 144, 7, 7, generator=g), torch.rand(64, 1, 7, 7, generator=g)
    t = torch.randint(1, 16, (64,), generator=g)
    w = torch.ones(16)
    w[0] = 0
    logits, loss, _, _, _ = O.train_step(cls, sd, x1, x2, t, w)
    return sd, x1, x2, t, w, _tup(logits), float(loss)


@pytest.mark.parametrize("cls", list(N_KEYS))
def test_mdlrs_gpu_b64_houston_shape_against_the_oracle(cls):
    _need_gpu()
    from vitcnn_amd import mdlrs
    sd, x1, x2, t, w, logits, loss = _b64_case(cls)
    m = getattr(mdlrs, cls)(144, 1, 16)
    m.load_state_dict(sd)
    m = m.to("cuda").train()
    hl, hloss, hg = _step(m, cls, x1, x2, t, w)
    _check_logits_loss(f"{cls} b64", hl, hloss, logits, loss)
    assert all(torch.isfinite(g).all() for g in hg.values())


def test_mdlrs_fused_adam_matches_torch_adam_and_gradients_repeat():
    """get_model's optimizer for the four nets (the fused vc_adamw with weight_decay 0) against torch.optim.Adam(lr
    1e-3) fed this path's gradients, five eager steps of Cross_fusion_CNN; repeating a step from the same state gives
    the same gradient bits (every sum of the backward runs in a fixed order)"""
    _need_gpu()
    from vitcnn_amd.optim import AdamW
    name, cls = "mdlrs_cross_b", "Cross_fusion_CNN"
    sd, _, _, t = golden(name)
    m = build(name)
    m.load_state_dict(sd)
    m = m.to("cuda").train()
    ref = {k: v.detach().clone() for k, v in m.named_parameters()}
    ref_params = [torch.nn.Parameter(v) for v in ref.values()]
    topt = torch.optim.Adam(ref_params, lr=1e-3)
    opt = AdamW(m.parameters(), lr=1e-3, weight_decay=0.0)
    for it in range(5):
        opt.zero_grad()
        _step(m, cls, t["x1"], t["x2"], t["target"], t["weight"])
        g1 = m.flat_params.grad.clone()
        if it == 0:
            # the repeat starts from the same state: the running statistics are buffers, not inputs of the gradient
            opt.zero_grad()
            _step(m, cls, t["x1"], t["x2"], t["target"], t["weight"])
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


# ---------------------------------------------------------------------------------------------- plugin surface
SCENE_W, SCENE_H, SCENE_P, SCENE_C1, SCENE_C2, SCENE_CLS = 23, 247, 7, 5, 1, 4


@functools.lru_cache(maxsize=None)
def _scene():
    """a 23 x 247 scene of three classes in blocks (label 0 = unlabelled), each with its own spectrum + noise:
    (23 - 6) * (247 - 6) = 4097 windows, so test() -- which sends min(4096, n) windows through the model at a time --
    ends on a batch of exactly one window"""
    g = torch.Generator().manual_seed(11)
    xs, ys = torch.meshgrid(torch.arange(SCENE_W), torch.arange(SCENE_H), indexing="ij")
    gt = 1 + ((xs // 8 + ys // 19) % 3)
    gt[torch.rand(SCENE_W, SCENE_H, generator=g) < 0.5] = 0
    proto = torch.rand(SCENE_CLS, SCENE_C1 + SCENE_C2, generator=g)
    cube = proto[1 + ((xs // 8 + ys // 19) % 3)] + 0.1 * torch.randn(SCENE_W, SCENE_H, SCENE_C1 + SCENE_C2, generator=g)
    return cube[:, :, :SCENE_C1].numpy().copy(), cube[:, :, SCENE_C1:].numpy().copy(), gt.numpy().astype(np.int64)


@pytest.mark.parametrize("cls", ["Cross_fusion_CNN", "Late_fusion_CNN"])
def test_mdlrs_train_and_test_plugin_surface(cls, tmp_path, monkeypatch):
    """two epochs of train() over a PatchBatcher (the eager TrainStepper path) reduce the loss and write a checkpoint
    with the reference's key set; test() returns [W, H, n_classes] equal to the eval forward of every window, the last
    of which travels alone (B = 1: logits stay [1, n_classes])"""
    _need_gpu()
    from vitcnn_amd import model_utils as mu
    from vitcnn_amd.window import PatchBatcher, window_count
    monkeypatch.chdir(tmp_path)
    img1, img2, gt = _scene()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m, opt, crit, kw = mu.get_model(cls, n_classes=SCENE_CLS, n_bands=(SCENE_C1, SCENE_C2), ignored_labels=[0],
                                    dataset="synthetic", device=dev)
    assert kw["patch_size"] == SCENE_P
    loader = PatchBatcher(img1, img2, gt, SCENE_P, ignored_labels=(0,), batch_size=64, device=dev, seed=0)
    nb = len(loader)
    assert nb >= 4
    mu.train("t", 0, None, m, opt, crit, loader, 2, device=dev, display_iter=0)
    st = mu.train.last_stats
    assert st["launch"] == "eager" and len(st["losses"]) == 2 * nb
    first, second = float(np.mean(st["losses"][:nb])), float(np.mean(st["losses"][nb:]))
    print(f"{cls}: mean loss of epoch 1 {first:.4f}, of epoch 2 {second:.4f}")
    assert np.isfinite(st["losses"]).all() and second < first, st["losses"]
    ck = [p for p in (tmp_path / "checkpoints").rglob("*.pth") if "final_epoch" in str(p)]
    assert ck
    loaded = torch.load(ck[0], map_location="cpu")
    ref_keys = list(golden("mdlrs_cross_a" if cls == "Cross_fusion_CNN" else "mdlrs_late_a")[0].keys())
    assert list(loaded.keys()) == ref_keys and len(ref_keys) == N_KEYS[cls]
    assert all(loaded[k].shape == v.shape for k, v in m.state_dict().items())
    # whole-image inference
    n = window_count(SCENE_W, SCENE_H, SCENE_P, 1)
    assert n == 4097 and n % 4096 == 1
    hp = dict(kw, n_classes=SCENE_CLS, batch_size=64, test_stride=1)
    probs = mu.test(0, m, img1, img2, hp)
    assert probs.shape == (SCENE_W, SCENE_H, SCENE_CLS)

    def windows(img):
        t = torch.from_numpy(img).permute(2, 0, 1)
        return t.unfold(1, SCENE_P, 1).unfold(2, SCENE_P, 1).permute(1, 2, 0, 3, 4).reshape(n, -1, SCENE_P, SCENE_P)

    b1, b2 = windows(img1).contiguous().cuda(), windows(img2).contiguous().cuda()
    m.eval()
    ref = []
    with torch.no_grad():
        for k0 in list(range(0, n - 1, 1000)) + [n - 1]:      # another grouping than test()'s; the last window alone
            k1 = min(k0 + 1000, n - 1) if k0 < n - 1 else n
            out = _tup(m(b1[k0:k1], b2[k0:k1]))[0]
            assert out.shape == (k1 - k0, SCENE_CLS)
            ref.append(out.cpu())
    ref = torch.cat(ref)
    p = SCENE_P // 2
    got = torch.from_numpy(probs[p:SCENE_W - p, p:SCENE_H - p].reshape(n, SCENE_CLS))
    assert _rel(got.float(), ref) < 1e-5, _rel(got.float(), ref)
    border = np.ones((SCENE_W, SCENE_H), dtype=bool)
    border[p:SCENE_W - p, p:SCENE_H - p] = False
    assert not probs[border].any()
