"""FusAtNet with `precision="bf16_store"` (the bf16 operands of every 3x3 conv contraction stored in memory; DESIGN.md
section 30) on the MI355X, held to what tests/test_fusat_bf16_gpu.py holds `"bf16"` to: the CPU's own execution of the
same arithmetic (tests/fusat_bf16_oracle.py), the same batch (B = 16, `torch.rand`, generator seed 2), and the same
bounds and margin rule (section 25's table): the logits within 3 x dev(E32, E64) of the float64 oracle, every
gradient tensor within 3 x its E32 deviation plus the 1e-5 max|grad| floor (at most 2 % of the tensors may need the
floor), and the argmax of every sample whose E64 top-2 margin exceeds 2 * 3 * dev(E32, E64) * max|E64|.  On the CPU the
oracle alone keeps 8 of the 16 samples above that margin for this seed (section 25); the test asks for the 4 that
test_fusat_bf16_gpu.py asks for and prints the count.  The eval-mode output is held to the same rules against the
eval-mode oracle pair.

Also here: three TrainStepper steps give equal losses eager and captured, `set_precision` between "bf16" and
"bf16_store" drops the captured graph, and "fp32" / "bf16" outputs are bit-equal before and after a "bf16_store"
forward on the same model.
"""
import pytest
import torch
import torch.nn.functional as F

import fusat_bf16_oracle as R

# the slowest item is the fixture (two CPU oracle forward + backward passes, one of them float64, two eval forwards and
# two GPU passes): the budget of tests/test_fusat_bf16_gpu.py, whose fixture runs more of them
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(21)]
DEV = "cuda"
B, SEED = 16, 2
MODE = "bf16_store"


def _seeded(precision="fp32"):
    from vitcnn_amd.fusatnet import FusAtNet
    torch.manual_seed(0)
    return FusAtNet(144, 1, 16, precision=precision)


def dev(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def _cpu(sd, x1, x2, t, w, dtype, train=True):
    """(logits, {name: gradient}) of the bf16-operand oracle in `dtype`, float64 on return; eval: no gradients"""
    P = {k: (v.to(dtype) if v.is_floating_point() else v).clone()
         .requires_grad_(train and v.is_floating_point() and "running" not in k) for k, v in sd.items()}
    with torch.set_grad_enabled(train):
        lg = R.forward(P, x1.to(dtype), x2.to(dtype), train=train, rounding=True)
        if train:
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
    out["E64"], out["G64"] = _cpu(sd, x1, x2, t, w, torch.float64)
    out["E32"], out["G32"] = _cpu(sd, x1, x2, t, w, torch.float32)
    out["V64"], _ = _cpu(sd, x1, x2, t, w, torch.float64, train=False)
    out["V32"], _ = _cpu(sd, x1, x2, t, w, torch.float32, train=False)
    out["spread"], out["vspread"] = dev(out["E32"], out["E64"]), dev(out["V32"], out["V64"])
    print("FIXTURE train dev(E32,E64) %.3e  eval dev(E32,E64) %.3e" % (out["spread"], out["vspread"]))
    assert out["spread"] > 1e-3   # the yardstick is a spread, not a tight bound in disguise
    crit = _crit(w)
    for prec in ("fp32", "bf16", MODE):
        m = _seeded(prec).to(DEV).train()
        assert m.precision == prec
        logits = m(x1.to(DEV), x2.to(DEV))
        crit(logits, t.to(DEV)).backward()
        torch.cuda.synchronize()
        out[prec] = dict(logits=logits.detach().cpu().double(), grads=_flat_grads(m))
    m = _seeded(MODE).to(DEV).eval()
    with torch.no_grad():
        out["eval"] = m(x1.to(DEV), x2.to(DEV)).cpu().double()
    return out


def test_mode_is_in_effect(runs):
    for other in ("fp32", "bf16"):   # not bit-identical to "bf16": another k order inside an MFMA
        assert not torch.equal(runs[MODE]["logits"], runs[other]["logits"]), other
    assert not any(torch.equal(runs[MODE]["grads"][k], runs["fp32"]["grads"][k])
                   for k in ("hfe.conv1.conv.weight", "mfe.conv1.conv.weight", "cm.conv5.conv.weight"))


def test_logits_are_the_same_arithmetic(runs):
    d, spread = dev(runs[MODE]["logits"], runs["E64"]), runs["spread"]
    print("LOGITS dev(HIP_bf16_store,E64) %.3e  dev(HIP_bf16,E64) %.3e  dev(E32,E64) %.3e  bound %.3e" %
          (d, dev(runs["bf16"]["logits"], runs["E64"]), spread, 3 * spread))
    assert d <= 3 * spread


def test_gradients_are_the_same_arithmetic(runs):
    """per parameter tensor: |HIP - E64| <= 3 |E32 - E64| + 1e-5 max|grad|; at most 2 % of the tensors may need the
    floor"""
    G64, G32, got = runs["G64"], runs["G32"], runs[MODE]["grads"]
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


def _argmax_rule(E64, got, spread):
    top2 = torch.sort(E64, dim=1).values[:, -2:]
    sel = (top2[:, 1] - top2[:, 0]) > 2 * 3 * spread * float(E64.abs().max())
    return int(sel.sum()), torch.equal(got.argmax(1)[sel], E64.argmax(1)[sel])


def test_argmax_where_the_margin_allows(runs):
    n, same = _argmax_rule(runs["E64"], runs[MODE]["logits"], runs["spread"])
    print("ARGMAX qualifying", n)
    assert n >= 4
    assert same


def test_eval_output_is_the_same_arithmetic(runs):
    d, spread = dev(runs["eval"], runs["V64"]), runs["vspread"]
    n, same = _argmax_rule(runs["V64"], runs["eval"], spread)
    print("EVAL dev(HIP_bf16_store,E64) %.3e  dev(E32,E64) %.3e  bound %.3e  argmax qualifying %d" %
          (d, spread, 3 * spread, n))
    assert d <= 3 * spread
    assert same


def _stepped(runs, use_graph, switch=None):
    from vitcnn_amd.optim import AdamW
    from vitcnn_amd.step import TrainStepper
    m = _seeded(MODE).to(DEV).train()
    opt = AdamW(m.parameters(), lr=1e-3, weight_decay=0.0)
    stepper = TrainStepper(m, opt, _crit(runs["w"]), capture_step=True, use_graph=use_graph)
    assert stepper.generic
    batch = (runs["x1"].to(DEV), runs["x2"].to(DEV), runs["t"].to(DEV))
    losses, graphs = [], []
    for i in range(3):
        losses.append(stepper.step(*batch).clone())
        graphs.append(len(stepper.graphs))
    for prec in switch or ():   # a captured graph recorded one mode's launches: dropped when the precision changes
        m.set_precision(prec)
        losses.append(stepper.step(*batch).clone())
        graphs.append(len(stepper.graphs))
    torch.cuda.synchronize()
    return torch.stack(losses), m.flat_params.detach().clone(), graphs, stepper.launch


def test_captured_steps_equal_eager_steps(runs):
    la, pa, ga, launch = _stepped(runs, True)
    lb, pb, gb, _ = _stepped(runs, False)
    assert launch == "hipGraph" and ga == [0, 1, 1] and gb == [0, 0, 0], (launch, ga)
    assert torch.equal(la, lb) and torch.equal(pa, pb)
    assert len(set(la.tolist())) == 3


def test_precision_change_drops_the_captured_graph(runs):
    la, pa, ga, launch = _stepped(runs, True, switch=("bf16", MODE))
    lb, pb, gb, _ = _stepped(runs, False, switch=("bf16", MODE))
    assert launch == "hipGraph" and ga == [0, 1, 1, 0, 0], (launch, ga)
    assert torch.equal(la, lb) and torch.equal(pa, pb)


def test_other_modes_are_untouched_by_a_bf16_store_forward(runs):
    x1, x2 = runs["x1"].to(DEV), runs["x2"].to(DEV)
    m = _seeded().to(DEV).eval()
    with torch.no_grad():
        before = {p: m.set_precision(p)(x1, x2).clone() for p in ("fp32", "bf16")}
        mid = m.set_precision(MODE)(x1, x2).clone()
        after = {p: m.set_precision(p)(x1, x2).clone() for p in ("fp32", "bf16")}
    for p in before:
        assert torch.equal(before[p], after[p]), p
        assert not torch.equal(before[p], mid), p


def test_measurement_routes_refuse_bf16_store(runs, monkeypatch):
    """the im2col + vc_gemm measurement route is fp32 only: the mode raises at program build"""
    from vitcnn_amd import fusatnet
    monkeypatch.setattr(fusatnet, "_TAP_CONV", False)
    m = _seeded(MODE).to(DEV).train()
    with pytest.raises(RuntimeError, match="bf16_store"):
        m(runs["x1"][:2].to(DEV), runs["x2"][:2].to(DEV))
