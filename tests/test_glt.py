"""GLT-Net on the MI355X path against the reference fixtures (tests/golden/gen_glt_golden.py) and the float64 oracle
(tests/glt_oracle.py): outputs, loss and every gradient, the BatchNorm bookkeeping of the shared convs, dropout with the
HIP path's masks fed to the oracle, bit-identical repeats, eval, and the plugin surface (get_model -> PatchBatcher ->
train() eager and captured -> test())."""
import functools

import numpy as np
import pytest
import torch

import glt_oracle as O
from glt_cases import CASES, build, grad_rule_fraction, load
from helpers import cpu_masks, program_spy

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHARED = ("cnn_encoder.conv1.1.num_batches_tracked", "cnn_encoder.conv2.1.num_batches_tracked")


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _model(name, state=None, p_drop=0.0):
    m = build(name, p_zero=False)
    if state is not None:
        m.load_state_dict(state)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = p_drop
    return m.to(DEV).train()


def _flat_grads(m):
    flat = m.flat_params.grad
    named = dict(m.named_parameters())
    return {n: flat[o:o + named[n].numel()].view(named[n].shape).cpu() for n, o in m._poff.items()}


def _step(m, x1, x2, t, w):
    from vitcnn_amd.losses import GLT_Loss
    out = m(x1.to(DEV), x2.to(DEV))
    loss = GLT_Loss(weight=w.float().to(DEV))(out, t.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return out[0].detach().cpu(), float(out[1].detach()), float(loss.detach()), _flat_grads(m)


def _check_step(tag, got, ref_cls, ref_con, ref_loss, ref_grads):
    cls, con, loss, grads = got
    ref_con, ref_loss = float(ref_con), float(ref_loss)
    frac, where = grad_rule_fraction(grads, ref_grads)
    print(f"GLT {tag}: x_cls rel {rel(cls, ref_cls):.3e}, con_loss rel {abs(con - ref_con) / ref_con:.3e}, loss rel "
          f"{abs(loss - ref_loss) / abs(ref_loss):.3e}, worst gradient {where} at {frac:.4f} of the rule")
    assert torch.isfinite(cls).all()
    assert rel(cls, ref_cls) < 1e-3
    assert abs(con - ref_con) <= 1e-3 * ref_con
    assert abs(loss - ref_loss) <= 1e-3 * abs(ref_loss)
    assert set(grads) == set(ref_grads)
    assert frac <= 1.0, (where, frac)
    for k, g in grads.items():      # the transformers' skipcat convolutions are never used: exactly zero
        if ".skipcat." in k:
            assert not bool(g.any()), k


def _check_buffers(m, ref_running):
    bufs = dict(m.named_buffers())
    for k, v in ref_running.items():
        if k.endswith("num_batches_tracked"):
            assert int(bufs[k]) == int(v) == (3 if k in SHARED else 1), k
        else:
            assert float((bufs[k].cpu().double() - v.double()).abs().max()) <= 1e-6, k


@pytest.mark.parametrize("name", list(CASES))
def test_glt_gpu_golden(name):
    """training forward / backward against the reference's float64 twin, then eval against its eval outputs"""
    t = load(name)
    m = _model(name, t["state"])
    got = _step(m, t["x1"], t["x2"], t["target"], t["weight"])
    _check_step(name, got, t["x_cls"], t["con_loss"], t["loss"], t["grads"])
    _check_buffers(m, t["running"])
    m.eval()
    with torch.no_grad():
        ev, econ = m(t["x1"].to(DEV), t["x2"].to(DEV))
    ev, econ = ev.cpu(), float(econ)
    print(f"GLT {name} eval: x_cls rel {rel(ev, t['eval_x_cls']):.3e}, con_loss {econ:.6f} / {float(t['eval_con_loss']):.6f}")
    assert rel(ev, t["eval_x_cls"]) < 1e-3
    assert torch.equal(ev.argmax(1), t["eval_x_cls"].argmax(1))
    assert abs(econ - float(t["eval_con_loss"])) <= 1e-3 * float(t["eval_con_loss"])
    _check_buffers(m, t["running"])     # eval updates nothing


@functools.lru_cache(maxsize=None)
def _b5():
    """B = 5 inputs for the glt_b model (an odd batch, more blocks than the fixtures')"""
    g = torch.Generator().manual_seed(50)
    return (torch.rand(5, 11, 12, 12, generator=g), torch.rand(5, 2, 12, 12, generator=g),
            torch.randint(1, 12, (5,), generator=g))


def test_glt_against_the_oracle_at_b5():
    t = load("glt_b")
    x1, x2, tg = _b5()
    m = _model("glt_b", t["state"])
    got = _step(m, x1, x2, tg, t["weight"])
    cls, con, loss, grads, rec = O.train_step(t["state"], x1, x2, tg, t["weight"])
    _check_step("B=5", got, cls, con, loss, grads)
    ref = dict(rec["running"])
    ref.update({k: torch.tensor(v) for k, v in rec["nbt"].items()})
    _check_buffers(m, ref)


def test_glt_against_the_oracle_with_band_counts_that_are_multiples_of_4():
    """8 + 4 bands: the decoder convolutions then run on the pipelined up-conv kernel (the fixtures' 30, 1, 11 and 2
    bands take the 128-wide one), and the crops' rows have no padding columns"""
    from vitcnn_amd.glt import GLT
    from glt_cases import REGISTRY
    torch.manual_seed(3)
    m = GLT(l1=8, l2=4, patch_size=4, num_patches=16, num_classes=7, en_depth=1, de_depth=1,
            **dict(REGISTRY, dropout=0.0, emb_dropout=0.0))
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(84)
    x1, x2 = torch.rand(3, 8, 12, 12, generator=g), torch.rand(3, 4, 12, 12, generator=g)
    tg, w = torch.randint(0, 7, (3,), generator=g), torch.ones(7)
    got = _step(m.to(DEV).train(), x1, x2, tg, w)
    cls, con, loss, grads, _ = O.train_step(state, x1, x2, tg, w)
    _check_step("8 + 4 bands", got, cls, con, loss, grads)


def test_glt_dropout_with_the_hip_masks_fed_to_the_oracle():
    t = load("glt_b")
    x1, x2, tg = _b5()
    m = _model("glt_b", t["state"], p_drop=0.1)
    from vitcnn_amd.glt import GLT
    with program_spy(GLT) as progs:
        got = _step(m, x1, x2, tg, t["weight"])
    masks = cpu_masks(progs[-1])
    assert set(masks) == set(O.sites(t["state"]))
    keep = torch.cat([v.reshape(-1) for v in masks.values()])
    assert 0.85 < float(keep.mean()) < 0.95
    drop = {k: (v, 0.1) for k, v in masks.items()}
    cls, con, loss, grads, _ = O.train_step(t["state"], x1, x2, tg, t["weight"], drop=drop)
    _check_step("dropout 0.1", got, cls, con, loss, grads)
    plain = O.train_step(t["state"], x1, x2, tg, t["weight"])[0]
    assert rel(got[0], plain) > 1e-4      # the masks did something


def test_glt_two_backward_runs_are_bit_identical():
    t = load("glt_a")
    m = _model("glt_a", t["state"])
    _step(m, t["x1"], t["x2"], t["target"], t["weight"])
    g1 = m.flat_params.grad.clone()
    m.zero_grad()
    m.load_state_dict(t["state"])       # the running statistics too: the same forward
    m = m.to(DEV).train()
    _step(m, t["x1"], t["x2"], t["target"], t["weight"])
    assert torch.equal(m.flat_params.grad, g1)


def test_glt_unused_parameters_stay_bit_unchanged_under_the_fused_adam():
    from vitcnn_amd.optim import AdamW
    t = load("glt_a")
    m = _model("glt_a", t["state"])
    opt = AdamW(m.parameters(), lr=5e-4, weight_decay=0.0)
    for _ in range(2):
        opt.zero_grad()
        _step(m, t["x1"], t["x2"], t["target"], t["weight"])
        opt.step()
    torch.cuda.synchronize()
    moved = 0.0
    for k, p in m.named_parameters():
        if ".skipcat." in k:
            assert torch.equal(p.detach().cpu(), t["state"][k]), k
        else:
            moved = max(moved, float((p.detach().cpu() - t["state"][k]).abs().max()))
    assert moved > 1e-4


SW, SH, SC1, SC2, SCLS, SP = 40, 42, 11, 2, 4, 12


@functools.lru_cache(maxsize=None)
def _scene():
    """a 40 x 42 scene of 3 classes in blocks, 11 HSI bands + 2 LiDAR bands in [0, 1], most pixels unlabelled"""
    g = torch.Generator().manual_seed(11)
    xs, ys = torch.meshgrid(torch.arange(SW), torch.arange(SH), indexing="ij")
    cls = 1 + ((xs // 5 + ys // 6) % 3)
    gt = cls.clone()
    gt[torch.rand(SW, SH, generator=g) < 0.7] = 0
    proto = torch.rand(SCLS, SC1 + SC2, generator=g)
    cube = (0.8 * proto[cls] + 0.2 * torch.rand(SW, SH, SC1 + SC2, generator=g)).clamp(0, 1)
    return cube[:, :, :SC1].numpy().copy(), cube[:, :, SC1:].numpy().copy(), gt.numpy().astype(np.int64)


def _train3(capture, tmp_path, monkeypatch):
    from vitcnn_amd import GLT, GLT_Loss
    from vitcnn_amd import model_utils as mu
    from vitcnn_amd.window import PatchBatcher
    monkeypatch.chdir(tmp_path)
    img1, img2, gt = _scene()
    dev = torch.device(DEV)
    torch.manual_seed(0)
    m, opt, crit, kw = mu.get_model("GLT_Net", n_classes=SCLS, n_bands=(SC1, SC2), ignored_labels=[0],
                                    dataset="synthetic", device=dev, patch_size=SP)
    assert isinstance(m, GLT) and isinstance(crit, GLT_Loss) and (kw["patch_size"], m.patch_size) == (SP, SP // 3)
    for mod in m.modules():     # dropout off: the two paths then compute the same numbers
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    probe = PatchBatcher(img1, img2, gt, SP, ignored_labels=(0,), batch_size=64, device=dev, seed=0)
    bs = -(-len(probe.centers) // 3)
    loader = PatchBatcher(img1, img2, gt, SP, ignored_labels=(0,), batch_size=bs, device=dev, seed=0)
    assert len(loader) == 3
    mu.train("t", 0, None, m, opt, crit, loader, 1, device=dev, display_iter=0, capture_step=capture)
    st = mu.train.last_stats
    return m, kw, [float(v) for v in st["losses"]], st["launch"]


def test_glt_train_eager_and_captured_and_test(tmp_path, monkeypatch):
    """get_model -> PatchBatcher at patch 12 (P = 4) -> 3 steps of train(), eager and with capture_step=True: the same
    per-step losses; then test() on the scene equals the model applied per window"""
    from vitcnn_amd import model_utils as mu
    m, kw, eager, launch_e = _train3(False, tmp_path, monkeypatch)
    _, _, captured, launch_c = _train3(True, tmp_path, monkeypatch)
    print(f"GLT train: eager {eager} ({launch_e}), captured {captured} ({launch_c})")
    assert launch_e == "eager" and launch_c == "hipGraph"
    assert len(eager) == len(captured) == 3 and np.isfinite(eager).all()
    for a, b in zip(eager, captured):
        assert abs(a - b) <= 1e-6 * abs(a), (eager, captured)
    img1, img2, _ = _scene()
    hp = dict(kw, n_classes=SCLS, batch_size=64, test_stride=1)
    probs = mu.test(0, m, img1, img2, hp)
    assert probs.shape == (SW, SH, SCLS)
    nx, ny = SW - SP + 1, SH - SP + 1
    n = nx * ny

    def windows(img):
        t = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).permute(2, 0, 1)
        return t.unfold(1, SP, 1).unfold(2, SP, 1).permute(1, 2, 0, 3, 4).reshape(n, -1, SP, SP)

    b1, b2 = windows(img1).contiguous().to(DEV), windows(img2).contiguous().to(DEV)
    m.eval()
    with torch.no_grad():
        ref = torch.cat([m(b1[k:k + 200], b2[k:k + 200])[0].cpu() for k in range(0, n, 200)])
    p = SP // 2
    got = torch.from_numpy(probs[p:p + nx, p:p + ny].reshape(n, SCLS))
    assert rel(got.float(), ref) < 1e-5, rel(got.float(), ref)
    rest = probs.copy()
    rest[p:p + nx, p:p + ny] = 0
    assert not rest.any()      # nothing lands outside the centres
