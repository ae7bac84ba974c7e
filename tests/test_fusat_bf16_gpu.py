"""FusAtNet with `precision="bf16"` (bf16 operands on every 3x3 conv contraction, fp32 accumulation; DESIGN.md
section 25) on the MI355X against the CPU's own execution of the same arithmetic (tests/fusat_bf16_oracle.py).

The net amplifies rounding: a chain of 29 train-mode BatchNorms, the last over 1x1 maps.  Two correct executions of the
SAME bf16-operand arithmetic -- the oracle in fp32 (E32) and in float64 (E64) -- differ by 4.6e-2 of the logits' norm
on this batch, so the model level is held to that spread (x3, the margin tests/test_muufl_gpu.py gives one fp32
execution over a float64 one), and the sharp checks are at the kernel level (tests/test_fusat_bf16_kernels_gpu.py).

The batch: B = 16, `torch.rand` inputs as test_fusatnet.py's B = 16 test, generator seed 2.  Measured on the CPU for
that seed (tests/fusat_bf16_oracle.py): dev(E32, E64) = 4.61e-2, dev(E64, F64) = 1.20e-1 (the mode's real
distance from fp32), dev(AC, F64) = 1.58e-1 to 1.64e-1 (the oracle under torch.autocast(bfloat16), whose result moves
with the CPU thread count); 8 of the 16 samples have an E64 top-2 margin above 2 * 3 * dev(E32, E64) * max|E64| =
0.316 (the margins next to it: 0.336 above, 0.207 below; seeds 11, 3, 4, 7, 13 leave 4 or fewer).  On the MI355X: dev(HIP bf16, E64) = 4.44e-2, the worst
gradient tensor at 2.11 x its E32 deviation, dev(HIP bf16, F64) = 1.17e-1.  A second fp32 execution of the oracle (the
batch reversed) needs the gradient floor for none of the 142 parameter tensors, and neither does the HIP run.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fusat_bf16_oracle as R
from oracle import fusat_oracle as O

# the slowest item is the fixture (five CPU oracle passes, two of them float64 forward + backward, and two GPU passes):
# 3 s to 7 s measured, depending on the host's CPU threads; every test's own GPU work is under 2 s.  3 x 7 s.
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(21)]
DEV = "cuda"
B, SEED = 16, 2


def _seeded(precision="fp32"):
    from vitcnn_amd.fusatnet import FusAtNet
    torch.manual_seed(0)
    return FusAtNet(144, 1, 16, precision=precision)


def dev(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def _cpu(sd, x1, x2, t, w, dtype, rounding, grads=True, autocast=False):
    """(logits, {name: gradient}) of the oracle in `dtype`, float64 on return"""
    P = {k: (v.to(dtype) if v.is_floating_point() else v).clone()
         .requires_grad_(grads and v.is_floating_point() and "running" not in k) for k, v in sd.items()}
    with torch.set_grad_enabled(grads):
        if autocast:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                lg = O.forward(P, x1.to(dtype), x2.to(dtype), train=True).float()
        else:
            lg = R.forward(P, x1.to(dtype), x2.to(dtype), train=True, rounding=rounding)
        if grads:
            F.cross_entropy(lg, t, weight=w.to(lg.dtype)).backward()
    return lg.detach().double(), {k: v.grad.double() for k, v in P.items() if v.requires_grad}


def _flat_grads(m):
    g = m.flat_params.grad.detach().cpu().double()
    named = dict(m.named_parameters())
    return {k: g[o:o + named[k].numel()].view(named[k].shape) for k, o in m._poff.items()}


def _crit(w):
    from vitcnn_amd.losses import CrossEntropyLoss
    return CrossEntropyLoss(weight=w.to(DEV))


@pytest.fixture(scope="module")
def runs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sd = {k: v.clone() for k, v in _seeded().state_dict().items()}
    g = torch.Generator().manual_seed(SEED)
    x1, x2 = torch.rand(B, 144, 11, 11, generator=g), torch.rand(B, 1, 11, 11, generator=g)
    t = torch.randint(1, 16, (B,), generator=g)
    w = torch.ones(16)
    w[0] = 0
    out = dict(x1=x1, x2=x2, t=t, w=w)
    out["E64"], out["G64"] = _cpu(sd, x1, x2, t, w, torch.float64, True)
    out["E32"], out["G32"] = _cpu(sd, x1, x2, t, w, torch.float32, True)
    out["F64"], _ = _cpu(sd, x1, x2, t, w, torch.float64, False, grads=False)
    out["F32"], _ = _cpu(sd, x1, x2, t, w, torch.float32, False, grads=False)
    out["AC"], _ = _cpu(sd, x1, x2, t, w, torch.float32, False, grads=False, autocast=True)
    out["spread"] = dev(out["E32"], out["E64"])
    print("FIXTURE dev(E32,E64) %.3e dev(E64,F64) %.3e dev(AC,F64) %.3e" %
          (out["spread"], dev(out["E64"], out["F64"]), dev(out["AC"], out["F64"])))
    # the yardstick is a spread, not a tight bound in disguise
    assert out["spread"] > 1e-3
    crit = _crit(w)
    for prec in ("fp32", "bf16"):
        m = _seeded(prec).to(DEV).train()
        assert m.precision == prec
        logits = m(x1.to(DEV), x2.to(DEV))
        crit(logits, t.to(DEV)).backward()
        torch.cuda.synchronize()
        out[prec] = dict(logits=logits.detach().cpu().double(), grads=_flat_grads(m))
    return out


def test_fp32_mode_is_unchanged(runs):
    d = dev(runs["fp32"]["logits"], runs["F32"])
    print("HIP fp32 vs fp32 oracle %.3e" % d)
    assert d < 1e-3


def test_bf16_is_in_effect(runs):
    assert not torch.equal(runs["bf16"]["logits"], runs["fp32"]["logits"])
    assert not any(torch.equal(runs["bf16"]["grads"][k], runs["fp32"]["grads"][k])
                   for k in ("hfe.conv1.conv.weight", "mfe.conv1.conv.weight", "cm.conv5.conv.weight"))


def test_bf16_logits_are_the_same_arithmetic(runs):
    d, spread = dev(runs["bf16"]["logits"], runs["E64"]), runs["spread"]
    print("LOGITS dev(HIP_bf16,E64) %.3e  dev(E32,E64) %.3e  bound %.3e" % (d, spread, 3 * spread))
    assert d <= 3 * spread


def test_bf16_gradients_are_the_same_arithmetic(runs):
    """per parameter tensor: |HIP - E64| <= 3 |E32 - E64| + 1e-5 max|grad| (test_muufl_gradients' floor); at most 2 %
    of the tensors may need the floor"""
    G64, G32, got = runs["G64"], runs["G32"], runs["bf16"]["grads"]
    assert set(got) == set(G64)
    floor = 1e-5 * max(float(v.abs().max()) for v in G64.values())
    bad, floored, worst = [], [], 0.0
    for k, g64 in G64.items():
        err, err32 = float((got[k] - g64).norm()), float((G32[k] - g64).norm())
        worst = max(worst, err / max(err32, 1e-300))
        if err > 3 * err32:
            floored.append((k, err, err32))
        if err > 3 * err32 + floor:
            bad.append((k, err, err32, float(g64.norm())))
    print("GRADS tensors %d, need the floor %d, fail %d, worst err/err32 %.3g, floor %.3e" %
          (len(G64), len(floored), len(bad), worst, floor), floored[:8])
    assert not bad, bad[:5]
    assert len(floored) <= 0.02 * len(G64), floored[:8]


def test_bf16_is_no_worse_than_the_reference_bf16(runs):
    d, ac = dev(runs["bf16"]["logits"], runs["F64"]), dev(runs["AC"], runs["F64"])
    print("VS FP32 dev(HIP_bf16,F64) %.3e  dev(AC,F64) %.3e" % (d, ac))
    assert d <= 1.5 * ac


def test_bf16_argmax_where_the_margin_allows(runs):
    E64, got = runs["E64"], runs["bf16"]["logits"]
    top2 = torch.sort(E64, dim=1).values[:, -2:]
    sel = (top2[:, 1] - top2[:, 0]) > 2 * 3 * runs["spread"] * float(E64.abs().max())
    print("ARGMAX qualifying", int(sel.sum()))
    assert int(sel.sum()) >= 4
    assert torch.equal(got.argmax(1)[sel], E64.argmax(1)[sel])


def _train(prec, runs, steps):
    from vitcnn_amd.optim import AdamW
    m = _seeded(prec).to(DEV).train()
    opt = AdamW(m.parameters(), lr=1e-3, weight_decay=0.0)
    crit = _crit(runs["w"])
    x1, x2, t = runs["x1"].to(DEV), runs["x2"].to(DEV), runs["t"].to(DEV)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = crit(m(x1, x2), t)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    return torch.stack(losses).cpu().tolist()


def test_bf16_trains(runs):
    """30 fused Adam steps on the fixed batch: fp32 trains, and bf16 costs at most 2x in steps"""
    a, b = _train("fp32", runs, 30), _train("bf16", runs, 30)
    print("TRAIN fp32", a[0], a[14], a[-1], "bf16", b[0], b[14], b[-1])
    assert a[-1] < a[0]
    assert b[-1] < a[14]


def _stepped(runs, use_graph, switch=False):
    from vitcnn_amd.optim import AdamW
    from vitcnn_amd.step import TrainStepper
    m = _seeded("bf16").to(DEV).train()
    opt = AdamW(m.parameters(), lr=1e-3, weight_decay=0.0)
    stepper = TrainStepper(m, opt, _crit(runs["w"]), capture_step=True, use_graph=use_graph)
    assert stepper.generic
    batch = (runs["x1"].to(DEV), runs["x2"].to(DEV), runs["t"].to(DEV))
    losses, graphs = [], []
    for i in range(3):
        losses.append(stepper.step(*batch).clone())
        graphs.append(len(stepper.graphs))
    if switch:   # the captured graph recorded bf16 launches: dropped when the precision changes
        m.set_precision("fp32")
        losses.append(stepper.step(*batch).clone())
        graphs.append(len(stepper.graphs))
    torch.cuda.synchronize()
    return torch.stack(losses), m.flat_params.detach().clone(), graphs, stepper.launch


def test_bf16_captured_steps_equal_eager_steps(runs):
    la, pa, ga, launch = _stepped(runs, True)
    lb, pb, gb, _ = _stepped(runs, False)
    assert launch == "hipGraph" and ga == [0, 1, 1] and gb == [0, 0, 0], (launch, ga)
    assert torch.equal(la, lb) and torch.equal(pa, pb)
    assert len(set(la.tolist())) == 3


def test_precision_change_drops_the_captured_graph(runs):
    la, pa, ga, launch = _stepped(runs, True, switch=True)
    lb, pb, gb, _ = _stepped(runs, False, switch=True)
    assert launch == "hipGraph" and ga == [0, 1, 1, 0], (launch, ga)
    assert torch.equal(la, lb) and torch.equal(pa, pb)


def test_measurement_routes_refuse_bf16(runs, monkeypatch):
    """the im2col + vc_gemm measurement route is fp32 only: bf16 raises at program build, fp32 runs"""
    from vitcnn_amd import fusatnet
    monkeypatch.setattr(fusatnet, "_TAP_CONV", False)
    x1, x2 = runs["x1"][:2].to(DEV), runs["x2"][:2].to(DEV)
    m = _seeded("bf16").to(DEV).train()
    with pytest.raises(RuntimeError, match="bf16"):
        m(x1, x2)
    with torch.no_grad():
        assert bool(torch.isfinite(m.set_precision("fp32")(x1, x2)).all())


def test_bf16_whole_image_inference():
    """model_utils.test() on a 15 x 14 scene, patch 11 (20 windows): the bf16 model's batched eval forward per window"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vitcnn_amd import model_utils as mu
    rng = np.random.default_rng(7)
    W, H, P = 15, 14, 11
    img1 = rng.random((W, H, 144), dtype=np.float32)
    img2 = rng.random((W, H, 1), dtype=np.float32)
    torch.manual_seed(0)
    model, _, _, hp = mu.get_model("FusAtNet", n_classes=16, n_bands=(144, 1), ignored_labels=[0], dataset="synthetic",
                                   device=torch.device(DEV), precision="bf16")
    assert model.precision == "bf16" and hp["patch_size"] == P
    hp["test_stride"] = 1
    probs = mu.test(0, model, img1, img2, hp)
    assert probs.dtype == np.float64 and probs.shape == (W, H, 16)
    wins = [(x, y) for x in range(W - P + 1) for y in range(H - P + 1)]
    x1 = torch.from_numpy(np.stack([img1[x:x + P, y:y + P].transpose(2, 0, 1) for x, y in wins])).to(DEV)
    x2 = torch.from_numpy(np.stack([img2[x:x + P, y:y + P].transpose(2, 0, 1) for x, y in wins])).to(DEV)
    model.eval()
    with torch.no_grad():
        lg = model(x1, x2).cpu().double().numpy()
        model.set_precision("fp32")
        lg32 = model(x1, x2).cpu().double().numpy()
    ref = np.zeros((W, H, 16))
    for (x, y), row in zip(wins, lg):
        ref[x + P // 2, y + P // 2] += row
    assert np.array_equal(probs, ref)
    assert not np.array_equal(lg, lg32)   # and it is the bf16 model that ran
