"""The captured step of the comparison models, the parts that need no GPU: the seed's Python
restatement, the new entry points in the header, which TrainStepper combinations `capture_step=True` accepts (decided
at construction, without touching a device) and train()'s signature."""
import ctypes
import inspect

import torch


def test_step_seed_is_deterministic_and_below_2_62():
    from vitcnn_amd import seeds
    base = 0x0123456789ABCDEF
    a = [seeds.step_seed(base, n) for n in range(1, 1001)]
    assert a == [seeds.step_seed(base, n) for n in range(1, 1001)]
    assert all(0 <= v < 1 << 62 for v in a) and len(set(a)) == 1000
    assert a[:3] != [seeds.step_seed(base + 1, n) for n in range(1, 4)]
    # the restatement itself: splitmix64 of (base + step * golden) mod 2^64, shifted right by 2
    z = (base + 7 * 0x9E3779B97F4A7C15) % (1 << 64)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % (1 << 64)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % (1 << 64)
    assert seeds.step_seed(base, 7) == (z ^ (z >> 31)) >> 2
    # the largest seed plus the largest site offset of any model stays below 2^63: the device sum never wraps
    assert (1 << 62) - 1 + seeds.site_offset(64) < 1 << 63


def test_host_seed_is_one_draw_with_the_rank_mixed_in(monkeypatch):
    from vitcnn_amd import parallel, seeds
    torch.manual_seed(5)
    first = int(torch.randint(0, 2 ** 62, (1,)))
    second = int(torch.randint(0, 2 ** 62, (1,)))
    torch.manual_seed(5)
    assert seeds.host_seed() == first                                   # rank 0: the draw itself
    assert int(torch.randint(0, 2 ** 62, (1,))) == second               # exactly one draw was consumed
    monkeypatch.setattr(parallel, "rank", lambda: 1)
    torch.manual_seed(5)
    assert seeds.host_seed() == (first + seeds.GOLDEN) % 2 ** 62
    assert int(torch.randint(0, 2 ** 62, (1,))) == second


def test_new_entry_points_parse_from_the_header():
    from vitcnn_amd._lib import parse_header
    sigs = parse_header()
    assert sigs["vc_seed_next"] == [ctypes.c_void_p, ctypes.c_void_p]
    for name in ("vc_dropout_fwd", "vc_sf_embed_fwd", "vc_hct_tokpool_fwd", "vc_hct_encoder_fwd", "vc_hct_ctattn_fwd"):
        old, new = sigs[name], sigs[name + "_ds"]
        i = old.index(ctypes.c_ulonglong)
        assert old.count(ctypes.c_ulonglong) == 1
        # the seed scalar becomes (pointer to the device seed, site offset); every other argument keeps its place
        assert new == old[:i] + [ctypes.c_void_p, ctypes.c_ulonglong] + old[i + 1:], name


def _hct():
    from vitcnn_amd.hctnet import HCTnet
    torch.manual_seed(0)
    return HCTnet(num_classes=12, num_tokens=4, heads=8)


def test_capture_step_eligibility_is_reported_in_launch():
    from vitcnn_amd import AdamW, CrossEntropyLoss
    from vitcnn_amd.s2eft import ViT
    from vitcnn_amd.step import TrainStepper
    lin = torch.nn.Linear(4, 3)
    st = TrainStepper(lin, torch.optim.SGD(lin.parameters(), lr=0.1), torch.nn.CrossEntropyLoss(), capture_step=True)
    assert not st.generic and not st.fused and not st.replays
    assert st.launch.startswith("eager (capture_step: ") and "comparison models" in st.launch
    m = _hct()
    st = TrainStepper(m, torch.optim.Adam(m.parameters(), lr=1e-4), CrossEntropyLoss(), capture_step=True)
    assert not st.generic and st.launch.startswith("eager (capture_step: ") and "optimizer" in st.launch
    st = TrainStepper(m, AdamW(m.parameters(), lr=1e-4), torch.nn.CrossEntropyLoss(), capture_step=True)
    assert not st.generic and st.launch.startswith("eager (capture_step: ") and "criterion" in st.launch
    other = _hct()
    st = TrainStepper(m, AdamW(other.parameters(), lr=1e-4), CrossEntropyLoss(), capture_step=True)
    assert not st.generic and "optimizer" in st.launch
    one = ViT(image_size=3, near_band=1, num_patches=8, num_classes=5, dim=16, depth=1, heads=2, mlp_dim=8)
    st = TrainStepper(one, AdamW(one.parameters(), lr=1e-4), CrossEntropyLoss(), capture_step=True)
    assert not st.generic and "two inputs" in st.launch
    # eligible: decided without a device; and the default keeps today's eager path
    opt, crit = AdamW(m.parameters(), lr=1e-4), CrossEntropyLoss()
    st = TrainStepper(m, opt, crit, capture_step=True)
    assert st.generic and st.replays and not st.fused and st.launch == "hipGraph" and st.capture_step
    st = TrainStepper(m, opt, crit, capture_step=True, use_graph=False)
    assert st.generic and st.launch == "eager"
    st = TrainStepper(m, opt, crit)
    assert not st.generic and not st.replays and st.launch == "eager" and not st.capture_step


def test_train_signature_keeps_every_parameter_and_adds_capture_step_last():
    from vitcnn_amd import model_utils as mu
    ps = inspect.signature(mu.train).parameters
    assert list(ps) == ["savename", "run", "bands", "net", "optimizer", "criterion", "data_loader", "epoch", "scheduler",
                        "display_iter", "device", "display", "val_loader", "supervision", "capture_step"]
    assert ps["capture_step"].default is False and ps["supervision"].default == "full"
    assert ps["display_iter"].default == 100 and ps["scheduler"].default is None
    sp = inspect.signature(mu._stepper).parameters
    assert list(sp) == ["net", "optimizer", "criterion", "capture_step"] and sp["capture_step"].default is False
