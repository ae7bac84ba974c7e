"""MHST with conv="mfma" (the pyramidal convolutions through vc_mhst_pconv_*) on the MI355X: the reference fixtures
through test_mhst.py's own bounds (the reference's numbers, not the direct path's); the launch trace against the recorded
"direct" one, call for call; captured steps against eager ones and a mode change after a capture; state_dicts
interchangeable between the modes."""
import pytest
import torch

import launch_cases
from helpers import launch_trace
from mhst_cases import CASES, load
from test_mhst import BASE, DEV, _check_after, _check_step, _model, _step, rel

pytestmark = pytest.mark.gpu

HOST_QUERIES = ("vc_mhst_pconv_ok", "vc_mhst_pconv_ws_floats")   # host arithmetic only: no launch behind them


@pytest.mark.parametrize("name", list(CASES))
def test_mhst_mfma_gpu_golden(name):
    t = load(name)
    m = _model(name, t["state"]).set_conv("mfma")
    got = _step(m, t["x1"], t["x2"], t["target"], t["weight"], noise=t["noise"])
    _check_step(name + " conv=mfma", got, t["out"], t["loss"], t["grads"])
    _check_after(m, t["x1"], t["x2"], t["running"], t["eval_out"])


def _substituted(call, ok, ws_floats):
    """what a recorded "direct" call becomes under "mfma": vc_mhst_conv_* at a whole-depth shape on the 8 x 8 map that
    vc_mhst_pconv_ok accepts -> vc_mhst_pconv_* with the same B, D, C, O, G, KS and strides (+ the workspace's size)"""
    name, a = call
    if name not in ("vc_mhst_conv_fwd", "vc_mhst_conv_dgrad", "vc_mhst_conv_wgrad"):
        return call
    B, D, H, W, C, O, G, KD, KS, sd, pd, Dout = a[:12]
    rest = a[12:]                                    # fwd: ldx, ldy; dgrad: lddy, lddx, beta; wgrad: ldx, lddy
    if (H, W, KD, sd, pd, Dout) != (8, 8, D, 1, 0, 1):
        return call
    ldx, ldy = (rest[1], rest[0]) if name.endswith("dgrad") else (rest[0], rest[1])
    if ok(D, C, O, G, KS, ldx, ldy) != 1:
        return call
    return [name.replace("vc_mhst_conv_", "vc_mhst_pconv_"), [B, D, C, O, G, KS] + rest + [ws_floats]]


def test_mfma_launch_trace_is_the_direct_one_with_the_pconv_calls_substituted():
    from vitcnn_amd._lib import lib
    want = launch_cases.fixture()["mhst_b"]
    ws_floats = [a[-1] for n, a in want if n == "vc_mhst_conv3_wgrad"][0]    # the program's one workspace
    want = [_substituted(c, lib().raw["vc_mhst_pconv_ok"], ws_floats) for c in want]
    count = lambda tr, n: sum(1 for c in tr if c[0] == n)   # noqa: E731
    # hsi_encoder.conv4 (4), lidar_encoder.conv2 (4), pyconv_classifier.conv1 (2); what stays direct: hsi_encoder.conv1,
    # the four spectral convs, lidar_encoder.conv1 (4)
    for d in ("fwd", "dgrad", "wgrad"):
        assert count(want, "vc_mhst_pconv_" + d) == 10
    assert count(want, "vc_mhst_conv_fwd") == 9 and count(want, "vc_mhst_conv_wgrad") == 9
    assert count(want, "vc_mhst_conv_dgrad") == 4      # only the spectral convs pass a gradient on

    torch.manual_seed(0)
    m, s1, s2 = launch_cases.CASES["mhst_b"]()
    m.set_conv("mfma")
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.1
    m = m.to(DEV).train()
    g = torch.Generator().manual_seed(5)
    x1 = torch.rand(launch_cases.B, *s1, generator=g).to(DEV)
    x2 = torch.rand(launch_cases.B, *s2, generator=g).to(DEV)
    torch.manual_seed(0)
    with launch_trace(lib()) as trace:
        m(x1, x2).sum().backward()
        torch.cuda.synchronize()
    got = [[n, list(a)] for n, a in trace if n not in HOST_QUERIES]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)     # the first call that differs
    assert got == want


def _stepper(conv, use_graph):
    from vitcnn_amd import CrossEntropyLoss, seeds
    from vitcnn_amd.optim import AdamW
    from vitcnn_amd.step import TrainStepper
    m = _model("mhst_b", load("mhst_b")["state"], p_drop=0.1).set_conv(conv)
    seeds.attach(m, BASE)
    opt = AdamW(m.parameters(), lr=8e-4)
    w = torch.ones(12, device=DEV)
    w[0] = 0.0
    return m, TrainStepper(m, opt, CrossEntropyLoss(weight=w), capture_step=True, use_graph=use_graph)


def _batches(n):
    g = torch.Generator().manual_seed(3)
    return [(torch.rand(4, 11, 8, 8, generator=g).to(DEV), torch.rand(4, 2, 8, 8, generator=g).to(DEV),
             torch.randint(1, 12, (4,), generator=g).to(DEV)) for _ in range(n)]


def test_mfma_captured_steps_equal_eager_steps_and_a_mode_change_re_records():
    from vitcnn_amd._lib import lib
    batches = _batches(3)
    res = {}
    for use_graph in (True, False):
        m, st = _stepper("mfma", use_graph)
        losses = [st.step(*b).clone() for b in batches[:2]]
        torch.cuda.synchronize()
        res[use_graph] = (torch.stack(losses), m.flat_params.detach().clone(), m, st)
    (la, pa, m, st), (lb, pb, _, sb) = res[True], res[False]
    assert st.launch == "hipGraph" and len(st.graphs) == 1 and sb.launch == "eager" and len(sb.graphs) == 0
    assert torch.equal(la, lb) and torch.equal(pa, pb)
    assert bool(torch.isfinite(la).all()) and float(la[0]) != float(la[1])
    # the captured graph launches the mfma family: after set_conv("direct") it must not be replayed
    m.set_conv("direct")
    with launch_trace(lib()) as trace:
        st.step(*batches[2])
        torch.cuda.synchronize()
    names = [n for n, _ in trace]
    assert len(st.graphs) == 0                       # dropped; this step ran eagerly and is re-recorded by the next
    assert not any(n.startswith("vc_mhst_pconv_") for n in names)
    whole_depth = [a for n, a in trace if n == "vc_mhst_conv_fwd" and a[7] == a[1] and a[8] > 1]
    assert len(whole_depth) >= 10                    # the pyramidal sites are back on the direct family


def test_modes_load_each_other_s_state_dict_and_agree_in_eval():
    t = load("mhst_b")
    a = _model("mhst_b", t["state"])
    b = _model("mhst_b").set_conv("mfma")
    assert a.conv == "direct" and b.conv == "mfma"
    b.load_state_dict(a.state_dict())
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    a.load_state_dict(b.state_dict())
    a.eval(), b.eval()
    with torch.no_grad():
        ya, yb = a(t["x1"].to(DEV), t["x2"].to(DEV)).cpu(), b(t["x1"].to(DEV), t["x2"].to(DEV)).cpu()
    print(f"MHST eval mfma against direct: rel {rel(yb, ya):.3e}")
    assert rel(yb, ya) < 1e-5
    assert b.conv == "mfma"      # the mode is no part of the state
