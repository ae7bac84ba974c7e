"""MHST comparison model on the MI355X: the HIP program against the reference fixtures (tests/golden/mhst_*.npz: the
reference's float64 twin fed the recorded gate noise, pinned to tests/mhst_oracle.py by tests/test_mhst_cpu.py) and
against that oracle at B = 64: output and loss within 1e-3 relative, argmax identical, every parameter gradient within
1e-3 of its norm + 1e-5 of the step's largest gradient norm (the rule of every comparison model), running statistics to
rtol 1e-3 / atol 1e-4, eval output within 1e-3 relative; a training step with dropout 0.1 and device-drawn gate noise,
the HIP path's masks, noise and decisions fed to the oracle; the fused AdamW step against torch.optim.AdamW; bit-identical
repeats; captured steps against eager ones; train() / test() through PatchBatcher at the even patch side 8.
"""
import functools

import numpy as np
import pytest
import torch

import mhst_oracle as O
from helpers import EPS32, TIE_ULPS, _audit_pool, _audit_relu, check_audit, cpu_masks, program_spy
from mhst_cases import CASES, REGISTRY, build, grad_rule_fraction, load

pytestmark = pytest.mark.gpu
DEV = "cuda"


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


def _step(m, x1, x2, t, w, noise=None):
    from vitcnn_amd.losses import CrossEntropyLoss
    out = m(x1.to(DEV), x2.to(DEV), gate_noise=noise)
    loss = CrossEntropyLoss(weight=w.float().to(DEV))(out, t.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().cpu(), float(loss.detach()), _flat_grads(m)


def _check_step(tag, got, ref_out, ref_loss, ref_grads):
    out, loss, grads = got
    ref_loss = float(ref_loss)
    frac, where = grad_rule_fraction(grads, ref_grads)
    print(f"MHST {tag}: out rel {rel(out, ref_out):.3e}, loss rel {abs(loss - ref_loss) / abs(ref_loss):.3e}, "
          f"worst gradient {where} at {frac:.4f} of the rule")
    assert torch.isfinite(out).all()
    assert rel(out, ref_out) < 1e-3
    assert torch.equal(out.argmax(1), ref_out.argmax(1))
    assert abs(loss - ref_loss) <= 1e-3 * abs(ref_loss)
    assert set(grads) == set(ref_grads)
    assert frac <= 1.0, (where, frac)


def _check_after(m, x1, x2, ref_running, ref_eval):
    bufs = dict(m.named_buffers())
    for k, v in ref_running.items():
        assert torch.allclose(bufs[k].cpu(), v.float(), rtol=1e-3, atol=1e-4), k
    assert all(int(v) == 1 for k, v in bufs.items() if k.endswith("num_batches_tracked"))
    m.eval()
    with torch.no_grad():
        ev = m(x1.to(DEV), x2.to(DEV)).cpu()
    m.train()
    print(f"MHST eval rel {rel(ev, ref_eval):.3e}")
    assert rel(ev, ref_eval) < 1e-3


@pytest.mark.parametrize("name", list(CASES))
def test_mhst_gpu_golden(name):
    t = load(name)
    m = _model(name, t["state"])
    got = _step(m, t["x1"], t["x2"], t["target"], t["weight"], noise=t["noise"])
    _check_step(name, got, t["out"], t["loss"], t["grads"])
    _check_after(m, t["x1"], t["x2"], t["running"], t["eval_out"])


def _audit_gates(audit, sel, rec, noise):
    """where an adopted gate decision differs from float64's own (v > 0), |v| must lie within TIE_ULPS fp32 ulps of the
    magnitude of what was summed into it ((|logits| + |noise|) / tau): the rule of helpers._audit_relu, per gate"""
    for i, v in rec["gate"].items():
        n = noise[i].double()
        differs = sel[i].double() != (v > 0).double()
        tie = TIE_ULPS * EPS32 * (n.abs() + (v * O.TAU - n).abs()) / O.TAU
        dist = float(v.abs()[differs].max()) if bool(differs.any()) else 0.0
        worst = float((v.abs()[differs] / tie[differs]).max()) if bool(differs.any()) else 0.0
        audit.append(dict(site=f"gate{i}", kind="gate", n=v.numel(), disagree=int(differs.sum()), dist=dist,
                          worst=worst, worst_ulp=worst))


def _adopted(prog):
    """the HIP program's ReLU and max-pool decisions as the oracle's `dec`, and what the audit needs of them"""
    d = prog.decisions()
    dec = dict(relu={k: (z > 0) for k, z in d["relu"].items()}, pool={k: a for k, (a, _) in d["pool"].items()})
    return dec, d


def _audit_relu_pool(audit, d, rec):
    for k, z in d["relu"].items():
        _audit_relu(audit, k, rec["pre"][k], z > 0, out=z)
    for k, (taps, vals) in d["pool"].items():
        _audit_pool(audit, k, rec["pool_in"][k], taps.to(torch.int64), vals)


def test_mhst_gpu_b64_144_bands_against_the_oracle():
    """the registry's model at 144 + 1 bands, B = 64 (no seed of 12 met the fixtures' conditions at this shape): the
    oracle adopts the HIP path's ReLU, max-pool and gate decisions, and every adopted decision that differs from
    float64's own must be an fp32 near-tie (TIE_ULPS, helpers._audit_relu / _audit_pool)"""
    from vitcnn_amd.mhst import MHST
    torch.manual_seed(0)
    m = MHST(**dict(CASES["mhst_a"], l1=144), **REGISTRY)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV).train()
    g = torch.Generator().manual_seed(5)
    B = 64
    x1, x2 = torch.rand(B, 144, 8, 8, generator=g), torch.rand(B, 1, 8, 8, generator=g)
    t = torch.randint(1, 16, (B,), generator=g)
    w = torch.ones(16)
    w[0] = 0
    u = torch.rand(8, B, 16, generator=g).clamp(1e-6, 1 - 1e-6)
    noise = (u.log() - (-u).log1p()).float()
    with program_spy(type(m)) as progs:
        got = _step(m, x1, x2, t, w, noise=noise)
    sel = progs[-1].sel.cpu()
    dec, d = _adopted(progs[-1])
    assert len(dec["relu"]) == 9 and len(dec["pool"]) == 2
    out, loss, grads, rec = O.train_step(state, x1, x2, t, w, noise, sel=sel, dec=dec)
    audit = []
    _audit_relu_pool(audit, d, rec)
    _audit_gates(audit, sel, rec, noise)
    summary = check_audit(audit, "mhst_b64")
    assert set(summary) == {"relu", "maxpool", "gate"}
    _check_step("b64 at 144 bands", got, out, loss, grads)
    after = dict(state, **rec["running"])
    _check_after(m, x1, x2, rec["running"], O.eval_forward(after, x1, x2))


def test_mhst_gpu_dropout_and_device_noise():
    """dropout 0.1 at every site and gate noise drawn on the device: the oracle evaluated with the HIP path's own keep
    masks, noise and decisions reproduces the step; eval afterwards applies none"""
    t = load("mhst_b")
    m = _model("mhst_b", t["state"], p_drop=0.1)
    with program_spy(type(m)) as progs:
        got = _step(m, t["x1"], t["x2"], t["target"], t["weight"])
    prog = progs[-1]
    masks = cpu_masks(prog)
    assert set(masks) == set(O.sites(t["state"]))
    keep = torch.cat([v.reshape(-1) for v in masks.values()])
    n = keep.numel()
    assert abs(keep.mean().item() - 0.9) <= 5 * (0.09 / n) ** 0.5, (keep.mean().item(), n)
    noise, sel = prog.noise.cpu(), prog.sel.cpu()
    assert bool(torch.isfinite(noise).all()) and float(noise.abs().max()) > 0
    drop = {k: (v, 0.1) for k, v in masks.items()}
    out, loss, grads, rec = O.train_step(t["state"], t["x1"], t["x2"], t["target"], t["weight"], noise, sel=sel,
                                         drop=drop)
    audit = []
    _audit_gates(audit, sel, rec, noise)    # the decisions the oracle adopted are its own, up to near-ties
    check_audit(audit, "mhst_dropout")
    _check_step("dropout", got, out, loss, grads)
    assert rel(out, t["out"]) > 1e-4   # masks and noise did something
    _check_after(m, t["x1"], t["x2"], rec["running"], O.eval_forward(dict(t["state"], **rec["running"]), t["x1"], t["x2"]))


def test_mhst_adamw_matches_torch_adamw_and_gradients_repeat():
    from vitcnn_amd.optim import AdamW
    t = load("mhst_b")
    m = _model("mhst_b", t["state"])
    ref = {k: v.detach().clone() for k, v in m.named_parameters()}
    ref_params = [torch.nn.Parameter(v) for v in ref.values()]
    topt = torch.optim.AdamW(ref_params, lr=8e-4)
    opt = AdamW(m.parameters(), lr=8e-4)
    opt.zero_grad()
    _step(m, t["x1"], t["x2"], t["target"], t["weight"], noise=t["noise"])
    g1 = m.flat_params.grad.clone()
    opt.zero_grad()
    _step(m, t["x1"], t["x2"], t["target"], t["weight"], noise=t["noise"])
    assert torch.equal(m.flat_params.grad, g1)      # two runs of the backward: the same bits
    grads = _flat_grads(m)
    for p, k in zip(ref_params, ref):
        p.grad = grads[k].to(DEV).clone()
    opt.step()
    topt.step()
    torch.cuda.synchronize()
    named = dict(m.named_parameters())
    moved = 0.0
    for p, k in zip(ref_params, ref):
        assert torch.allclose(named[k].detach(), p.detach(), rtol=1e-5, atol=1e-6), k
        moved = max(moved, float((p.detach() - t["state"][k].to(DEV)).abs().max()))
    assert moved > 1e-4


BASE = 0x1234567


def _run_steps(use_graph, batches):
    from vitcnn_amd import CrossEntropyLoss, seeds
    from vitcnn_amd.optim import AdamW
    from vitcnn_amd.step import TrainStepper
    m = _model("mhst_b", load("mhst_b")["state"], p_drop=0.1)
    st = seeds.attach(m, BASE)
    opt = AdamW(m.parameters(), lr=8e-4)
    w = torch.ones(12, device=DEV)
    w[0] = 0.0
    stepper = TrainStepper(m, opt, CrossEntropyLoss(weight=w), capture_step=True, use_graph=use_graph)
    losses = [stepper.step(*b).clone() for b in batches]
    torch.cuda.synchronize()
    out = {"loss": torch.stack(losses), "params": m.flat_params.detach().clone(), "grad": m.flat_params.grad.clone(),
           "m": opt._dev["m"].clone(), "v": opt._dev["v"].clone(), "step": opt._dev["step"].clone()}
    out.update({"buf." + k: v.clone() for k, v in m.named_buffers()})
    return out, stepper, st


def test_mhst_captured_steps_equal_eager_steps():
    """four steps with capture_step=True against the same stepper with use_graph=False: every bit of losses,
    parameters, buffers and moments; the masks and the gate noise are redrawn at every replay (the losses differ)"""
    from vitcnn_amd import seeds
    g = torch.Generator().manual_seed(3)
    batches = [(torch.rand(4, 11, 8, 8, generator=g).to(DEV), torch.rand(4, 2, 8, 8, generator=g).to(DEV),
                torch.randint(1, 12, (4,), generator=g).to(DEV)) for _ in range(4)]
    a, sa, seed_a = _run_steps(True, batches)
    b, sb, seed_b = _run_steps(False, batches)
    assert sa.launch == "hipGraph" and len(sa.graphs) == 1, sa.launch
    assert sb.launch == "eager" and len(sb.graphs) == 0
    want = (BASE, 4, seeds.step_seed(BASE, 4))
    assert seed_a.read() == want and seed_b.read() == want
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (k, float((a[k].double() - b[k].double()).abs().max()))
    assert bool(torch.isfinite(a["loss"]).all()) and len(set(a["loss"].tolist())) == 4
    assert bool(a["step"].any()) and bool(a["m"].any())


SW, SH, SC1, SC2, SCLS, SP = 40, 50, 11, 2, 4, 8


@functools.lru_cache(maxsize=None)
def _scene():
    """a 40 x 50 scene of 3 classes in blocks, 11 HSI bands + 2 LiDAR bands, a few unlabelled pixels"""
    g = torch.Generator().manual_seed(11)
    xs, ys = torch.meshgrid(torch.arange(SW), torch.arange(SH), indexing="ij")
    cls = 1 + ((xs // 5 + ys // 6) % 3)
    gt = cls.clone()
    gt[torch.rand(SW, SH, generator=g) < 0.1] = 0
    proto = torch.rand(SCLS, SC1 + SC2, generator=g)
    cube = proto[cls] + 0.1 * torch.randn(SW, SH, SC1 + SC2, generator=g)
    return cube[:, :, :SC1].numpy().copy(), cube[:, :, SC1:].numpy().copy(), gt.numpy().astype(np.int64)


def test_patchbatcher_even_patch_side_equals_the_reference_arithmetic():
    """datasets.py:550-581 at P = 8: the window of centre (x, y) is [x - 4, x + 4) x [y - 4, y + 4) and its label the
    window's [4, 4] element, i.e. gt[x, y]"""
    from vitcnn_amd.window import PatchBatcher
    img1, img2, gt = _scene()
    pb = PatchBatcher(img1, img2, gt, SP, ignored_labels=(0,), batch_size=32, device=DEV, seed=1)
    x1, x2, t = next(iter(pb))
    assert x1.shape == (32, SC1, SP, SP) and x2.shape == (32, SC2, SP, SP)
    for i in range(32):
        x, y = (int(v) for v in pb.centers[i])
        a, b = x - SP // 2, y - SP // 2
        assert a >= 0 and b >= 0 and a + SP <= SW and b + SP <= SH
        assert np.array_equal(x1[i].cpu().numpy(), img1[a:a + SP, b:b + SP].transpose(2, 0, 1).astype(np.float32))
        assert np.array_equal(x2[i].cpu().numpy(), img2[a:a + SP, b:b + SP].transpose(2, 0, 1).astype(np.float32))
        assert int(t[i]) == int(gt[a:a + SP, b:b + SP][SP // 2, SP // 2]) == int(gt[x, y])


def test_mhst_train_and_test_plugin_surface(tmp_path, monkeypatch):
    """two epochs of train() through PatchBatcher(patch_size=8) write a checkpoint with the reference's key set; test()
    returns [W, H, n_classes] whose window (x, y) lands on pixel (x + 4, y + 4) (model_utils.py:1127-1131 at an even
    side), equal to batched eval forwards on the windows"""
    from vitcnn_amd import model_utils as mu
    from vitcnn_amd.window import PatchBatcher
    monkeypatch.chdir(tmp_path)
    img1, img2, gt = _scene()
    dev = torch.device(DEV)
    torch.manual_seed(0)
    m, opt, crit, kw = mu.get_model("MHST", n_classes=SCLS, n_bands=(SC1, SC2), ignored_labels=[0], dataset="synthetic",
                                    device=dev)
    assert kw["patch_size"] == SP and isinstance(m, type(build("mhst_b")))
    for mod in m.modules():     # dropout off: only the gates' noise differs between the epochs
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    loader = PatchBatcher(img1, img2, gt, SP, ignored_labels=(0,), batch_size=64, device=dev, seed=0)
    nb = len(loader)
    assert nb >= 2
    mu.train("t", 0, None, m, opt, crit, loader, 2, device=dev, display_iter=0)
    st = mu.train.last_stats
    assert st["launch"] == "eager" and len(st["losses"]) == 2 * nb
    first, second = float(np.mean(st["losses"][:nb])), float(np.mean(st["losses"][nb:]))
    print(f"MHST: mean loss of epoch 1 {first:.5f}, of epoch 2 {second:.5f}")
    assert np.isfinite(st["losses"]).all() and second < first, st["losses"]
    ck = [p for p in (tmp_path / "checkpoints").rglob("*.pth") if "final_epoch" in str(p)]
    assert ck
    assert list(torch.load(ck[0], map_location="cpu").keys()) == load("mhst_a")["keys"]
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
        ref = torch.cat([m(b1[k:k + 200], b2[k:k + 200]).cpu() for k in range(0, n, 200)])
    p = SP // 2
    got = torch.from_numpy(probs[p:p + nx, p:p + ny].reshape(n, SCLS))
    assert rel(got.float(), ref) < 1e-5, rel(got.float(), ref)
    rest = probs.copy()
    rest[p:p + nx, p:p + ny] = 0
    assert not rest.any()      # nothing lands outside the centres


def test_mhst_input_rejections():
    m = _model("mhst_b")
    z = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
    for x1, x2 in ((z(2, 12, 8, 8), z(2, 2, 8, 8)),          # 12 HSI bands
                   (z(2, 11, 8, 8), z(2, 1, 8, 8)),          # 1 LiDAR band
                   (z(2, 11, 8, 8).cpu(), z(2, 2, 8, 8)),    # a CPU tensor
                   (z(2, 11, 7, 7), z(2, 2, 7, 7)),          # a patch side other than 8
                   (z(2, 11, 9, 9), z(2, 2, 9, 9)),
                   (z(2, 11, 8, 8), z(3, 2, 8, 8))):         # batch sizes differ
        with pytest.raises(RuntimeError):
            m(x1, x2)
    with pytest.raises(RuntimeError):
        m(z(2, 11, 8, 8), z(2, 2, 8, 8), gate_noise=z(2, 3, 16))
    m.eval()
    with torch.no_grad():
        assert m(z(1, 11, 8, 8), z(1, 2, 8, 8)).shape == (1, 12)
