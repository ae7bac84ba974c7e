"""MHST with conv="mfma_all" ("mfma" plus hsi_encoder.conv1 through vc_mhst_conv1_* and the four spectral convolutions
through vc_mhst_sconv_*) on the MI355X: the reference fixtures through test_mhst.py's own bounds (the reference's numbers,
not the other modes'); the launch trace against the recorded "direct" one, call for call; captured steps against eager
ones and mode changes after a capture; the gradient's bits; state_dicts interchangeable between the three modes."""
import pytest
import torch

import launch_cases
from helpers import launch_trace
from mhst_cases import CASES, load
from test_mhst import DEV, _check_after, _check_step, _model, _step, rel
from test_mhst_pconv_gpu import HOST_QUERIES, _batches, _stepper, _substituted

pytestmark = pytest.mark.gpu

QUERIES = HOST_QUERIES + ("vc_mhst_conv1_ws_floats", "vc_mhst_sconv_ws_floats")   # host arithmetic only
NEW = ("vc_mhst_conv1_", "vc_mhst_sconv_")


@pytest.mark.parametrize("name", list(CASES))
def test_mhst_mfma_all_gpu_golden(name):
    t = load(name)
    m = _model(name, t["state"]).set_conv("mfma_all")
    got = _step(m, t["x1"], t["x2"], t["target"], t["weight"], noise=t["noise"])
    _check_step(name + " conv=mfma_all", got, t["out"], t["loss"], t["grads"])
    _check_after(m, t["x1"], t["x2"], t["running"], t["eval_out"])


def _front(trace, ws_floats):
    """what an "mfma" trace becomes under "mfma_all": the (11, 3, 3, 5) vc_mhst_conv_fwd -> vc_mhst_conv1_fwd, the run of
    four KS = 1 forwards -> one vc_mhst_sconv_fwd, the four KS = 1 (wgrad, dgrad) pairs -> one vc_mhst_sconv_wgrad then one
    vc_mhst_sconv_dgrad with beta 0, the (11, 3, 3, 5) weight gradient -> vc_mhst_conv1_wgrad; each with the workspace"""
    out, i = [], 0
    shape = lambda a: tuple(a[7:11])   # noqa: E731  (KD, KS, sd, pd)
    while i < len(trace):
        name, a = trace[i]
        if name == "vc_mhst_conv_fwd" and shape(a) == (11, 3, 3, 5):
            B, l1, ldx, ldy = a[0], a[1], a[12], a[13]
            assert ldx == 1 and tuple(a[2:7]) == (8, 8, 1, 16, 1)
            out.append(["vc_mhst_conv1_fwd", [B, l1, ldy, ws_floats]])
        elif name == "vc_mhst_conv_wgrad" and shape(a) == (11, 3, 3, 5):
            out.append(["vc_mhst_conv1_wgrad", [a[0], a[1], a[13], ws_floats]])
        elif name == "vc_mhst_conv_fwd" and a[8] == 1:
            run = trace[i:i + 4]
            assert [c[0] for c in run] == ["vc_mhst_conv_fwd"] * 4 and [c[1][7] for c in run] == [1, 3, 5, 11]
            assert all(c[1][12:] == a[12:] and c[1][:2] == a[:2] for c in run)
            out.append(["vc_mhst_sconv_fwd", [a[0], a[1], a[12], a[13], ws_floats]])
            i += 3
        elif name == "vc_mhst_conv_wgrad" and a[8] == 1:
            run = trace[i:i + 8]
            assert [c[0] for c in run] == ["vc_mhst_conv_wgrad", "vc_mhst_conv_dgrad"] * 4
            assert [c[1][7] for c in run] == [1, 1, 3, 3, 5, 5, 11, 11]
            assert [c[1][14] for c in run[1::2]] == [0.0, 1.0, 1.0, 1.0]      # the betas of the four direct calls
            ldx, lddy = a[12], a[13]
            assert run[1][1][12:14] == [lddy, ldx]
            out.append(["vc_mhst_sconv_wgrad", [a[0], a[1], ldx, lddy, ws_floats]])
            out.append(["vc_mhst_sconv_dgrad", [a[0], a[1], lddy, ldx, 0.0, ws_floats]])
            i += 7
        else:
            out.append(trace[i])
        i += 1
    return out


def test_mfma_all_launch_trace_is_the_direct_one_with_the_calls_substituted():
    from vitcnn_amd._lib import lib
    want = launch_cases.fixture()["mhst_b"]
    ws_floats = [a[-1] for n, a in want if n == "vc_mhst_conv3_wgrad"][0]    # the program's one workspace
    want = _front([_substituted(c, lib().raw["vc_mhst_pconv_ok"], ws_floats) for c in want], ws_floats)
    count = lambda tr, n: sum(1 for c in tr if c[0] == n)   # noqa: E731
    for n in ("vc_mhst_conv1_fwd", "vc_mhst_conv1_wgrad", "vc_mhst_sconv_fwd", "vc_mhst_sconv_wgrad",
              "vc_mhst_sconv_dgrad"):
        assert count(want, n) == 1, n
    # what stays on the direct family: lidar_encoder.conv1 only
    assert count(want, "vc_mhst_conv_fwd") == 4 and count(want, "vc_mhst_conv_wgrad") == 4
    assert count(want, "vc_mhst_conv_dgrad") == 0
    for d in ("fwd", "dgrad", "wgrad"):
        assert count(want, "vc_mhst_pconv_" + d) == 10
    i = [c[0] for c in want].index("vc_mhst_sconv_wgrad")
    assert want[i + 1][0] == "vc_mhst_sconv_dgrad" and want[i + 1][1][4] == 0.0

    torch.manual_seed(0)
    m, s1, s2 = launch_cases.CASES["mhst_b"]()
    m.set_conv("mfma_all")
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
    got = [[n, list(a)] for n, a in trace if n not in QUERIES]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)     # the first call that differs
    assert got == want


def test_mfma_all_captured_steps_equal_eager_steps_and_mode_changes_re_record():
    from vitcnn_amd._lib import lib
    batches = _batches(4)
    res = {}
    for use_graph in (True, False):
        m, st = _stepper("mfma_all", use_graph)
        losses = [st.step(*b).clone() for b in batches[:2]]
        torch.cuda.synchronize()
        res[use_graph] = (torch.stack(losses), m.flat_params.detach().clone(), m, st)
    (la, pa, m, st), (lb, pb, _, sb) = res[True], res[False]
    assert st.launch == "hipGraph" and len(st.graphs) == 1 and sb.launch == "eager" and len(sb.graphs) == 0
    assert torch.equal(la, lb) and torch.equal(pa, pb)
    assert bool(torch.isfinite(la).all()) and float(la[0]) != float(la[1])
    # the captured graph launches the new families: after a mode change it must not be replayed
    for mode, batch in (("mfma", batches[2]), ("direct", batches[3])):
        m.set_conv(mode)
        with launch_trace(lib()) as trace:
            st.step(*batch)
            torch.cuda.synchronize()
        names = [n for n, _ in trace]
        assert len(st.graphs) == 0, mode                 # dropped; this step ran eagerly and is re-recorded by the next
        assert not any(n.startswith(NEW) for n in names), mode
        # the front of the HSI encoder is back on the direct family: conv1 and the four spectral convs
        assert sum(1 for n, a in trace if n == "vc_mhst_conv_fwd" and (a[8] == 1 or a[7:11] == [11, 3, 3, 5])) == 5, mode
        assert any(n.startswith("vc_mhst_pconv_") for n in names) == (mode == "mfma")
        st.step(*batch)                                  # re-recorded in the new mode


def test_mfma_all_gradient_bits_repeat():
    t = load("mhst_b")
    m = _model("mhst_b", t["state"]).set_conv("mfma_all")
    m.zero_grad()
    _step(m, t["x1"], t["x2"], t["target"], t["weight"], noise=t["noise"])
    g1 = m.flat_params.grad.clone()
    m.zero_grad()
    _step(m, t["x1"], t["x2"], t["target"], t["weight"], noise=t["noise"])
    assert bool(g1.any()) and torch.equal(m.flat_params.grad, g1)


def test_the_three_modes_load_each_other_s_state_dict_and_agree_in_eval():
    t = load("mhst_b")
    models = {"direct": _model("mhst_b", t["state"]), "mfma": _model("mhst_b").set_conv("mfma"),
              "mfma_all": _model("mhst_b").set_conv("mfma_all")}
    for a in models.values():
        for b in models.values():
            b.load_state_dict(a.state_dict())
    sd = [m.state_dict() for m in models.values()]
    assert all(list(s) == list(sd[0]) and all(torch.equal(s[k], sd[0][k]) for k in s) for s in sd)
    assert [m.conv for m in models.values()] == list(models)     # the mode is no part of the state
    x1, x2 = t["x1"].to(DEV), t["x2"].to(DEV)
    out = {}
    for k, m in models.items():
        m.eval()
        with torch.no_grad():
            out[k] = m(x1, x2).cpu()
    r = rel(out["mfma_all"], out["direct"])
    print(f"MHST eval mfma_all against direct at mhst_b: rel {r:.3e}")
    assert r < 1e-5


def test_mfma_all_agrees_with_direct_in_eval_at_144_bands():
    from vitcnn_amd import model_utils as mu
    args = dict(n_classes=16, n_bands=(144, 1), ignored_labels=[0], dataset="Houston2013", device=torch.device(DEV))
    torch.manual_seed(0)
    a = mu.get_model("MHST", **args)[0]
    torch.manual_seed(0)
    b = mu.get_model("MHST", **args, conv="mfma_all")[0]
    assert (a.conv, b.conv) == ("direct", "mfma_all")
    g = torch.Generator().manual_seed(11)
    x1, x2 = torch.rand(2, 144, 8, 8, generator=g).to(DEV), torch.rand(2, 1, 8, 8, generator=g).to(DEV)
    a.eval(), b.eval()
    with torch.no_grad():
        ya, yb = a(x1, x2).cpu(), b(x1, x2).cpu()
    r = rel(yb, ya)
    print(f"MHST eval mfma_all against direct at 144 + 1 bands, B = 2: rel {r:.3e}")
    assert bool(torch.isfinite(yb).all()) and r < 1e-5
