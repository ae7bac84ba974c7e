"""The captured training step of the comparison models on the MI355X (`TrainStepper(capture_step=True)`, DESIGN.md
section 23), step level, at tiny configurations with dropout 0.1:

* HCTnet B 4, patch 7, 12 classes, 4 tokens; MFT B 4, patch 7, 11 bands; SpectralFormer B 4, 8 + 1 bands: four steps on
  four different batches through the captured path (eager, capture + replay, replay, replay) and through the same
  stepper with `use_graph=False` give the same bits everywhere: losses, parameters, BatchNorm buffers, optimizer moments.
* after `.to()` re-packs the parameters the stale graph is dropped and captured again, with the all-eager run's bits.
* the masks are redrawn: one HCTnet site's mask bytes (5120 of them at B 16) after each of three replays equal the numpy
  restatement of the hash under `step_seed(base, n)`, lie within 5 sigma of keep fraction 1 - p, differ pairwise in a
  fraction within 5 sigma of 2 p (1 - p) (sigma = sqrt(p (1 - p) / N)), and the device step counter advanced by one
  per step.  BASE was checked on the CPU against both bands with the restatement alone (seed_cases.within_bands:
  keep 0.8971 / 0.9004 / 0.9055, differing 0.1799 / 0.1750, bands 0.9 +- 0.0210 and 0.18 +- 0.0210).
* without an attached seed a plain capture of the same model repeats its masks byte for byte (the behaviour this
  feature removes, pinned so the difference is visible).
* `train(..., capture_step=True)` over a tiny PatchBatcher scene reports "hipGraph", the short last batch has a graph
  of its own, and the same call without the keyword reports "eager".
"""
import numpy as np
import pytest
import torch

from helpers import program_spy
from pixel_cases import spectralformer
from seed_cases import HCT_ENC_SITE, hct_enc_attn_index, mix32_keep, within_bands

pytestmark = pytest.mark.gpu
DEV = "cuda"
BASE = 0x0123456789ABCDEF
P_DROP = 0.1


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _set_dropout(m, p):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = p
    return m


def _hct(ncls=12):
    from vitcnn_amd.hctnet import HCTnet
    return _set_dropout(HCTnet(num_classes=ncls, num_tokens=4, heads=8), P_DROP)


def _mft():
    from vitcnn_amd.mft import MFT
    return _set_dropout(MFT(patch_size=7, FM=16, NC=11, NCLidar=1, Classes=12, HSIOnly=False), P_DROP)


def _sf():
    return spectralformer(9, 12, P_DROP)


def _batches(kind, n, B, seed=3):
    g = torch.Generator().manual_seed(seed)
    shapes = {"hct": ((3, 7, 7), (1, 7, 7)), "mft": ((11, 7, 7), (1, 7, 7)), "sf": ((8,), (1,))}[kind]
    return [(torch.rand(B, *shapes[0], generator=g).to(DEV), torch.rand(B, *shapes[1], generator=g).to(DEV),
             torch.randint(1, 12, (B,), generator=g).to(DEV)) for _ in range(n)]


def _optimizer(kind, m):
    from vitcnn_amd.optim import Adam, AdamW
    if kind == "mft":
        return Adam(m.parameters(), lr=5e-4, weight_decay=5e-3)
    return AdamW(m.parameters(), lr=1e-3, weight_decay=0.0)


def _crit():
    from vitcnn_amd import CrossEntropyLoss
    w = torch.ones(12, device=DEV)
    w[0] = 0.0
    return CrossEntropyLoss(weight=w)


BUILD = {"hct": _hct, "mft": _mft, "sf": _sf}


def _run(kind, use_graph, batches):
    from vitcnn_amd import seeds
    from vitcnn_amd.step import TrainStepper
    torch.manual_seed(0)
    m = BUILD[kind]().to(DEV).train()
    st = seeds.attach(m, BASE)
    opt = _optimizer(kind, m)
    stepper = TrainStepper(m, opt, _crit(), capture_step=True, use_graph=use_graph)
    assert stepper.generic
    losses = [stepper.step(*b).clone() for b in batches]
    torch.cuda.synchronize()
    out = {"loss": torch.stack(losses), "params": m.flat_params.detach().clone(), "grad": m.flat_params.grad.clone(),
           "m": opt._dev["m"].clone(), "v": opt._dev["v"].clone(), "step": opt._dev["step"].clone()}
    out.update({"buf." + k: v.clone() for k, v in m.named_buffers()})
    return out, stepper, st


@pytest.mark.parametrize("kind", ["hct", "mft", "sf"])
def test_captured_steps_equal_eager_steps(kind):
    _need_gpu()
    from vitcnn_amd import seeds
    batches = _batches(kind, 4, 4)
    a, sa, seed_a = _run(kind, True, batches)
    b, sb, seed_b = _run(kind, False, batches)
    assert sa.launch == "hipGraph" and len(sa.graphs) == 1, sa.launch
    assert sb.launch == "eager" and len(sb.graphs) == 0
    want = (BASE, 4, seeds.step_seed(BASE, 4))
    assert seed_a.read() == want and seed_b.read() == want
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (kind, k, float((a[k].double() - b[k].double()).abs().max()))
    assert bool(torch.isfinite(a["loss"]).all()) and len(set(a["loss"].tolist())) == 4
    assert bool(a["step"].any()) and bool(a["m"].any())     # the optimizer stepped


def test_stale_graphs_are_dropped_after_a_reflatten():
    """`.to()` re-packs the parameters into a new flat buffer: the captured graph holds the old addresses and is dropped,
    the next batch runs eagerly, the one after is captured again; the results equal the all-eager run's bit for bit"""
    _need_gpu()
    from vitcnn_amd import seeds
    from vitcnn_amd.step import TrainStepper
    batches = _batches("hct", 6, 4)

    def run(use_graph):
        torch.manual_seed(0)
        m = _hct().to(DEV).train()
        seeds.attach(m, BASE)
        stepper = TrainStepper(m, _optimizer("hct", m), _crit(), capture_step=True, use_graph=use_graph)
        losses, graphs = [], []
        for i, b in enumerate(batches):
            if i == 3:
                m.to(DEV)
            losses.append(stepper.step(*b).clone())
            graphs.append(len(stepper.graphs))
        torch.cuda.synchronize()
        return torch.stack(losses), m.flat_params.detach().clone(), graphs, stepper.launch

    la, pa, ga, launch = run(True)
    lb, pb, gb, _ = run(False)
    assert launch == "hipGraph" and ga == [0, 1, 1, 0, 1, 1] and gb == [0] * 6
    assert torch.equal(la, lb) and torch.equal(pa, pb)


def test_replays_redraw_the_masks():
    _need_gpu()
    from vitcnn_amd import seeds
    from vitcnn_amd.step import TrainStepper
    B, T = 16, 5
    torch.manual_seed(0)
    m = _hct().to(DEV).train()
    st = seeds.attach(m, BASE)
    stepper = TrainStepper(m, _optimizer("hct", m), _crit(), capture_step=True)
    batches = _batches("hct", 4, B)
    masks, steps = [], []
    with program_spy(type(m)) as progs:   # every HCTnet forward's program (inside a capture: the graph's own buffers)
        for i, b in enumerate(batches):
            stepper.step(*b)
            torch.cuda.synchronize()
            steps.append(st.read()[1])
            if i >= 1:     # steps 2, 3, 4 are replays of the graph captured at step 2: its mask buffer is progs[1]'s
                assert len(progs) == 2
                masks.append(progs[1].masks["enc.h.attn"].cpu().numpy().copy())
    assert stepper.launch == "hipGraph" and len(stepper.graphs) == 1
    assert steps == [1, 2, 3, 4]
    assert masks[0].shape == (B, T, 64) and masks[0].size >= 4096
    idx = hct_enc_attn_index(B, T)
    for n, mk in zip((2, 3, 4), masks):
        want = mix32_keep(seeds.step_seed(BASE, n) + seeds.site_offset(HCT_ENC_SITE), idx, P_DROP)
        assert np.array_equal(mk, want), (n, int((mk != want).sum()))
    keep, diff, ok = within_bands(masks, P_DROP)
    print(f"keep fractions {keep}, differing fractions {diff}")
    assert ok, (keep, diff)


def test_a_plain_capture_repeats_its_masks():
    """no seed attached, the model captured as tools/hct_step.py does: the host seed is baked into the launches"""
    _need_gpu()
    from vitcnn_amd import seeds
    torch.manual_seed(0)
    m = _hct().to(DEV).train()
    assert seeds.state(m) is None
    opt, crit = _optimizer("hct", m), _crit()
    x1, x2, t = _batches("hct", 1, 16)[0]

    def step():
        crit(m(x1, x2), t).backward()
        opt.step()

    opt.zero_grad(set_to_none=True)
    step()
    torch.cuda.synchronize()
    opt.zero_grad(set_to_none=True)
    opt.sync_hyper()
    graph = torch.cuda.CUDAGraph()
    masks = []
    with program_spy(type(m)) as progs:
        with torch.cuda.graph(graph):
            step()
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()
            masks.append(progs[0].masks["enc.h.attn"].cpu().clone())
    assert 0 < int(masks[0].sum()) < masks[0].numel()
    assert torch.equal(masks[0], masks[1]) and torch.equal(masks[1], masks[2])


# ---------------------------------------------------------------------------------------------- train()
def _scene():
    """an 18 x 21 scene, every pixel labelled 1..3: (18 - 7) * (21 - 7) = 154 patch centres -> batches of 64, 64, 26"""
    g = torch.Generator().manual_seed(11)
    xs, ys = torch.meshgrid(torch.arange(18), torch.arange(21), indexing="ij")
    gt = 1 + ((xs // 4 + ys // 5) % 3)
    proto = torch.rand(4, 4, generator=g)
    cube = proto[gt] + 0.1 * torch.randn(18, 21, 4, generator=g)
    return cube[:, :, :3].numpy().copy(), cube[:, :, 3:].numpy().copy(), gt.numpy().astype(np.int64)


def _train_model(name):
    from vitcnn_amd.mdlrs import Early_fusion_CNN
    torch.manual_seed(0)
    return (Early_fusion_CNN(3, 1, 4) if name == "early" else _hct(4)).to(DEV)


@pytest.mark.parametrize("name", ["early", "hct"])
def test_train_with_capture_step(name, tmp_path, monkeypatch):
    _need_gpu()
    from vitcnn_amd import CrossEntropyLoss, model_utils as mu, seeds
    from vitcnn_amd.optim import AdamW
    from vitcnn_amd.window import PatchBatcher
    monkeypatch.chdir(tmp_path)
    img1, img2, gt = _scene()
    dev = torch.device(DEV)
    loader = PatchBatcher(img1, img2, gt, 7, ignored_labels=(0,), batch_size=64, device=dev, seed=0)
    nb = len(loader)
    sizes = [int(t.shape[0]) for _, _, t in loader]
    assert nb == 3 and sizes == [64, 64, 26]
    w = torch.ones(4, device=dev)
    w[0] = 0.0
    m = _train_model(name)
    opt, crit = AdamW(m.parameters(), lr=1e-3, weight_decay=0.0), CrossEntropyLoss(weight=w)
    mu.train("t", 0, None, m, opt, crit, loader, 2, device=dev, display_iter=0, capture_step=True)
    st = mu.train.last_stats
    assert st["launch"] == "hipGraph", st["launch"]
    assert len(st["losses"]) == 2 * nb and np.isfinite(st["losses"]).all()
    assert len(set(st["losses"])) == 2 * nb       # each recorded loss is its own step's (the replayed buffer was cloned)
    stepper = m._vc_stepper
    assert stepper.generic and len(stepper.graphs) == 2      # the full batches' graph and the short last batch's
    assert sorted(k[0][0] for k in stepper.graphs) == [26, 64]
    assert [p for p in (tmp_path / "checkpoints").rglob("*.pth") if "final_epoch" in str(p)]
    s = seeds.state(m)
    if name == "hct":
        assert s is not None and s.read()[1] == 2 * nb      # attached by the stepper, advanced once per step
    else:
        assert s is None                                    # no dropout: the same path without a seed
    # the same call without the keyword: today's eager path
    m2 = _train_model(name)
    opt2 = AdamW(m2.parameters(), lr=1e-3, weight_decay=0.0)
    mu.train("t", 1, None, m2, opt2, crit, loader, 2, device=dev, display_iter=0)
    st2 = mu.train.last_stats
    assert st2["launch"] == "eager" and len(st2["losses"]) == 2 * nb
    assert not m2._vc_stepper.generic and seeds.state(m2) is None
