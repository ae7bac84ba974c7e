"""HCTnet comparison model on the MI355X: the HIP path (csrc/hctnet.hip + the conv / norm / GEMM entry points) against
the reference module's fixtures (tests/golden/hctnet_a*.npz, hctnet_b*.npz) and against tests/hct_oracle.py (float64,
pinned to the same fixtures by tests/test_hctnet_cpu.py) at B = 64: logits and loss within 1e-3 relative, argmax
identical, every parameter gradient within 1e-3 of its norm + 1e-5 of the step's largest gradient norm (the rule of
test_s2eft.py / test_fusatnet.py / test_mft.py; it also bounds the three conv biases whose true gradient is zero
because a train-mode BatchNorm follows them), running statistics and eval logits; dropout 0.1 with the HIP path's own
keep masks fed to the oracle; the fused Adam step against torch.optim.Adam; train() through PatchBatcher(applyPCA=True)
and test().
"""
import functools

import numpy as np
import pytest
import torch

import hct_oracle as O
from hct_cases import KW, UNUSED, ZERO_GRAD_BIASES, golden, rel

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _model(kw, sd, p_drop=0.0):
    from vitcnn_amd.hctnet import HCTnet
    m = HCTnet(**kw)
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
    print(f"HCTnet {tag}: logits rel {rel(hl, ref_logits):.3e}, loss rel {abs(hloss - ref_loss) / abs(ref_loss):.3e}")
    assert torch.isfinite(hl).all()
    assert rel(hl, ref_logits) < 1e-3, rel(hl, ref_logits)
    assert torch.equal(hl.argmax(1), ref_logits.argmax(1))
    assert abs(hloss - ref_loss) <= 1e-3 * abs(ref_loss)
    gmax = max(float(g.double().norm()) for g in ref_grads.values())
    worst = ("", 0.0)
    assert set(hg) == set(ref_grads)
    for k, g in ref_grads.items():
        err = float((hg[k].double() - g.double()).norm())
        bound = 1e-3 * float(g.double().norm()) + 1e-5 * gmax
        worst = max(worst, (k, err / bound), key=lambda r: r[1])
        assert err <= bound, (k, err, float(g.double().norm()), gmax)
        if k.startswith(UNUSED):
            assert not hg[k].any(), k      # the unused transformer: exactly zero
    print(f"HCTnet {tag}: worst gradient {worst[0]} at {worst[1]:.4f} of the rule (gmax {gmax:.3e})")
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
    assert rel(le, ref_eval) < 1e-3, rel(le, ref_eval)
    m.train()


@pytest.mark.parametrize("name", list(KW))
def test_hctnet_gpu_golden(name):
    _need_gpu()
    sd, run, gr, t = golden(name)
    m = _model(KW[name], sd)
    got = _step(m, t["x1"], t["x2"], t["target"], t["weight"])
    _check_step(name, got, t["logits"], t["loss"], gr)
    _check_after(m, t["x1"], t["x2"], run, t["eval_logits"])


@functools.lru_cache(maxsize=None)
def _b64_case():
    """B = 64 at patch 11, 16 classes, 6 tokens: seeded initial state, inputs, and the float64 oracle's step"""
    from vitcnn_amd.hctnet import HCTnet
    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in HCTnet(**KW["hctnet_a"]).state_dict().items()}
    g = torch.Generator().manual_seed(5)
    x1, x2 = torch.rand(64, 3, 11, 11, generator=g), torch.rand(64, 1, 11, 11, generator=g)
    t = torch.randint(1, 16, (64,), generator=g)
    w = torch.ones(16)
    w[0] = 0
    logits, loss, grads, running, _ = O.train_step(sd, x1, x2, t, w)
    after = dict(sd, **running)
    return sd, x1, x2, t, w, logits, float(loss), grads, running, O.eval_logits(after, x1, x2)


def test_hctnet_gpu_b64_against_the_oracle():
    _need_gpu()
    sd, x1, x2, t, w, logits, loss, grads, running, ev = _b64_case()
    m = _model(KW["hctnet_a"], sd)
    _check_step("b64", _step(m, x1, x2, t, w), logits, loss, grads)
    _check_after(m, x1, x2, running, ev)


def test_hctnet_gpu_dropout_train():
    """dropout 0.1 at the reference's 12 sites: keep fraction ~0.9, logits and every gradient equal the oracle's
    evaluated with the HIP path's own keep masks; eval afterwards applies none"""
    _need_gpu()
    from helpers import cpu_masks, program_spy
    sd, run, _, t = golden("hctnet_a")
    m = _model(KW["hctnet_a"], sd, p_drop=0.1)
    with program_spy(type(m)) as progs:
        got = _step(m, t["x1"], t["x2"], t["target"], t["weight"])
    masks = cpu_masks(progs[-1])
    assert set(masks) == set(O.SITES) and len(masks) == 12
    keep = torch.cat([v.reshape(-1) for v in masks.values()])
    n = keep.numel()
    assert abs(keep.mean().item() - 0.9) <= 5 * (0.09 / n) ** 0.5, (keep.mean().item(), n)
    assert all(0.0 < v.mean().item() < 1.0 for v in masks.values())
    drop = {k: (v, 0.1) for k, v in masks.items()}
    logits, loss, grads, running, _ = O.train_step(sd, t["x1"], t["x2"], t["target"], t["weight"], drop=drop)
    _check_step("dropout", got, logits, float(loss), grads)
    assert rel(logits.float(), t["logits"]) > 1e-3   # the masks did something
    _check_after(m, t["x1"], t["x2"], run, t["eval_logits"])   # eval: the no-dropout forward


def test_hctnet_adam_matches_torch_adam_and_gradients_repeat():
    """get_model('HCTnet')'s optimizer (the fused AdamW with weight_decay 0 over the flat buffer) against
    torch.optim.Adam(lr 1e-4) fed the same gradients, one step; the unused transformer's parameters do not move by a
    bit; a second run of the same step gives the same gradient bits"""
    _need_gpu()
    from vitcnn_amd.optim import AdamW
    sd, _, _, t = golden("hctnet_b")
    m = _model(KW["hctnet_b"], sd)
    ref = {k: v.detach().clone() for k, v in m.named_parameters()}
    ref_params = [torch.nn.Parameter(v) for v in ref.values()]
    topt = torch.optim.Adam(ref_params, lr=1e-4)
    opt = AdamW(m.parameters(), lr=1e-4, weight_decay=0.0)
    opt.zero_grad()
    _step(m, t["x1"], t["x2"], t["target"], t["weight"])
    g1 = m.flat_params.grad.clone()
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
        if k.startswith(UNUSED):
            assert torch.equal(named[k].detach().cpu(), sd[k]), k
        else:
            moved = max(moved, float((p.detach() - sd[k].cuda()).abs().max()))
    assert moved > 5e-5


SCENE, SCENE_C1, SCENE_CLS, SCENE_P = 24, 8, 4, 11


@functools.lru_cache(maxsize=None)
def _scene():
    """a 24 x 24 scene of 3 classes in blocks, 8 HSI bands + 1 LiDAR band, a few unlabelled pixels"""
    g = torch.Generator().manual_seed(11)
    xs, ys = torch.meshgrid(torch.arange(SCENE), torch.arange(SCENE), indexing="ij")
    cls = 1 + ((xs // 4 + ys // 5) % 3)
    gt = cls.clone()
    gt[torch.rand(SCENE, SCENE, generator=g) < 0.1] = 0
    proto = torch.rand(SCENE_CLS, SCENE_C1 + 1, generator=g)
    cube = proto[cls] + 0.1 * torch.randn(SCENE, SCENE, SCENE_C1 + 1, generator=g)
    return cube[:, :, :SCENE_C1].numpy().copy(), cube[:, :, SCENE_C1:].numpy().copy(), gt.numpy().astype(np.int64)


def test_patchbatcher_apply_pca_equals_a_batcher_on_the_reduced_cube():
    _need_gpu()
    from vitcnn_amd.model_utils import apply_pca
    from vitcnn_amd.window import PatchBatcher
    img1, img2, gt = _scene()
    a = PatchBatcher(img1, img2, gt, SCENE_P, ignored_labels=(0,), batch_size=64, device="cuda", seed=3, applyPCA=True)
    b = PatchBatcher(apply_pca(img1, 3), img2, gt, SCENE_P, ignored_labels=(0,), batch_size=64, device="cuda", seed=3)
    c = PatchBatcher(img1, img2, gt, SCENE_P, ignored_labels=(0,), batch_size=64, device="cuda", seed=3)
    ba, bb = list(a), list(b)
    assert len(ba) == len(bb) == len(a) >= 2
    for (x1, x2, t), (y1, y2, u) in zip(ba, bb):
        assert x1.shape[1:] == (3, SCENE_P, SCENE_P) and x2.shape[1:] == (1, SCENE_P, SCENE_P)
        assert torch.equal(x1, y1) and torch.equal(x2, y2) and torch.equal(t, u)
    assert next(iter(c))[0].shape[1] == SCENE_C1     # the default is unchanged: no reduction


def test_hctnet_train_and_test_plugin_surface(tmp_path, monkeypatch):
    """two epochs of train() through PatchBatcher(applyPCA=True) (the eager path; dropout off, so the same batches
    repeat exactly and the loss must fall) write a checkpoint with the reference's key set; test() returns
    [W, H, n_classes] equal to batched eval forwards on the apply_pca'd windows"""
    _need_gpu()
    from vitcnn_amd import model_utils as mu
    from vitcnn_amd.window import PatchBatcher
    monkeypatch.chdir(tmp_path)
    img1, img2, gt = _scene()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m, opt, crit, kw = mu.get_model("HCTnet", n_classes=SCENE_CLS, n_bands=(SCENE_C1, 1), ignored_labels=[0],
                                    dataset="synthetic", device=dev)
    assert kw["patch_size"] == SCENE_P and kw["applyPCA"] is True
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    loader = PatchBatcher(img1, img2, gt, SCENE_P, ignored_labels=(0,), batch_size=64, device=dev, seed=0,
                          applyPCA=kw["applyPCA"])
    nb = len(loader)
    assert nb >= 2
    unused = {k: v.detach().clone() for k, v in m.named_parameters() if k.startswith(UNUSED)}
    mu.train("t", 0, None, m, opt, crit, loader, 2, device=dev, display_iter=0)
    st = mu.train.last_stats
    assert st["launch"] == "eager" and len(st["losses"]) == 2 * nb
    first, second = float(np.mean(st["losses"][:nb])), float(np.mean(st["losses"][nb:]))
    print(f"HCTnet: mean loss of epoch 1 {first:.5f}, of epoch 2 {second:.5f}")
    assert np.isfinite(st["losses"]).all() and second < first, st["losses"]
    named = dict(m.named_parameters())
    assert len(unused) == 12 and all(torch.equal(named[k].detach(), v) for k, v in unused.items())
    ck = [p for p in (tmp_path / "checkpoints").rglob("*.pth") if "final_epoch" in str(p)]
    assert ck
    loaded = torch.load(ck[0], map_location="cpu")
    assert list(loaded.keys()) == list(golden("hctnet_a")[0].keys())
    # whole-image inference
    hp = dict(kw, n_classes=SCENE_CLS, batch_size=64, test_stride=1)
    probs = mu.test(0, m, img1, img2, hp)
    assert probs.shape == (SCENE, SCENE, SCENE_CLS)
    side = SCENE - SCENE_P + 1
    n = side * side

    def windows(img):
        t = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).permute(2, 0, 1)
        return t.unfold(1, SCENE_P, 1).unfold(2, SCENE_P, 1).permute(1, 2, 0, 3, 4).reshape(n, -1, SCENE_P, SCENE_P)

    b1, b2 = windows(mu.apply_pca(img1, 3)).contiguous().cuda(), windows(img2).contiguous().cuda()
    m.eval()
    with torch.no_grad():
        ref = torch.cat([m(b1[k:k + 50], b2[k:k + 50]).cpu() for k in range(0, n, 50)])   # another grouping than test()'s
    p = SCENE_P // 2
    got = torch.from_numpy(probs[p:SCENE - p, p:SCENE - p].reshape(n, SCENE_CLS))
    assert rel(got.float(), ref) < 1e-5, rel(got.float(), ref)


def test_hctnet_input_rejections():
    _need_gpu()
    m = _model(KW["hctnet_b"], golden("hctnet_b")[0])
    z = lambda *s: torch.zeros(*s, device="cuda")
    for x1, x2 in ((z(2, 4, 7, 7), z(2, 1, 7, 7)),          # 4 HSI bands
                   (z(2, 3, 7, 7), z(2, 2, 7, 7)),          # 2 LiDAR bands
                   (z(2, 3, 7, 7).cpu(), z(2, 1, 7, 7)),    # a CPU tensor
                   (z(2, 3, 4, 4), z(2, 1, 4, 4)),          # a patch side below 5
                   (z(2, 3, 31, 31), z(2, 1, 31, 31)),      # and above 30
                   (z(2, 3, 7, 7), z(3, 1, 7, 7))):         # batch sizes differ
        with pytest.raises(RuntimeError):
            m(x1, x2)
    with torch.no_grad():
        assert m(z(2, 3, 5, 5), z(2, 1, 5, 5)).shape == (2, 12)     # the smallest patch: a 1 x 1 HSI map
