"""The comparison models' shared autograd bridge and counter pool (vitcnn_amd/program.py): a
backward through one output of a multi-output model equals the backward with explicit zero gradients for the others, a
forward under no_grad keeps no program and leaves the next training step alone, and the arrival counters are one array
per (device, stream).  Smallest shapes the models accept: every check here is about the bridge, not the kernels.

The launch sequence of the models built from `Program`'s shared helpers is pinned: one training forward + backward asks
the library for exactly the recorded calls (entry point and non-pointer arguments, in order; tests/launch_cases.py), so a
refactor of the shared host code that moves a launch, an argument or the workspace's size fails here."""
import gc
import weakref

import pytest
import torch

import launch_cases
from helpers import program_spy

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _one_output_against_explicit_zeros(m, x1, x2, n_out):
    """the flat gradient of a backward through outs[0] alone, and of one over the first n_out outputs with explicit zero
    gradients for all but outs[0] -- the same upstream gradient both times"""
    g = torch.Generator().manual_seed(3)
    outs = m(x1, x2)[:n_out]
    g0 = torch.randn(outs[0].shape, generator=g).to(DEV)
    outs[0].backward(g0)
    alone = m.flat_params.grad.clone()
    m.zero_grad()
    outs = m(x1, x2)[:n_out]
    torch.autograd.backward(outs, [g0] + [torch.zeros_like(o) for o in outs[1:]])
    torch.cuda.synchronize()
    return alone, m.flat_params.grad


def test_cross_fusion_backward_through_one_output_equals_explicit_zero_gradients():
    _need_gpu()
    from vitcnn_amd.mdlrs import P_MIN, Cross_fusion_CNN
    torch.manual_seed(0)
    m = Cross_fusion_CNN(5, 1, 3).to(DEV).train()
    x1, x2 = torch.randn(2, 5, P_MIN, P_MIN).to(DEV), torch.randn(2, 1, P_MIN, P_MIN).to(DEV)
    alone, explicit = _one_output_against_explicit_zeros(m, x1, x2, 3)
    assert alone.abs().max() > 0 and torch.isfinite(alone).all()
    assert torch.equal(alone, explicit)


def test_endnet_backward_through_out_alone_equals_explicit_zero_gradients():
    _need_gpu()
    from vitcnn_amd.endnet import EndNet
    torch.manual_seed(0)
    m = EndNet(5, 1, 3).to(DEV).train()
    x1, x2 = torch.randn(2, 5).to(DEV), torch.randn(2, 1).to(DEV)
    alone, explicit = _one_output_against_explicit_zeros(m, x1, x2, 3)   # (out, de_x1, de_x2)
    assert alone.abs().max() > 0 and torch.isfinite(alone).all()
    assert torch.equal(alone, explicit)


def test_no_grad_forward_keeps_no_program_and_a_training_step_follows():
    _need_gpu()
    from vitcnn_amd.endnet import EndNet
    torch.manual_seed(0)
    m = EndNet(5, 1, 3).to(DEV).train()
    x1, x2 = torch.randn(2, 5).to(DEV), torch.randn(2, 1).to(DEV)
    with program_spy(EndNet) as progs:
        with torch.no_grad():
            out = m(x1, x2)[0]
        assert len(progs) == 1 and not progs[0].needs_grad and not out.requires_grad
        kept = weakref.ref(progs.pop())
        gc.collect()
        assert kept() is None            # nothing but the spy held the no_grad forward's program
        out = m(x1, x2)[0]
        assert len(progs) == 1 and progs[0].needs_grad and out.requires_grad
        out.sum().backward()
    torch.cuda.synchronize()
    grad = m.flat_params.grad
    assert grad is not None and torch.isfinite(grad).all() and grad.abs().max() > 0


def test_counter_pool_is_one_array_per_device_and_stream():
    _need_gpu()
    from vitcnn_amd.program import counters
    dev = torch.device(DEV, torch.cuda.current_device())
    cur = torch.cuda.current_stream(dev).cuda_stream
    other = torch.cuda.Stream(dev)
    a = counters(dev, cur)
    assert a != 0 and counters(dev, cur) == a
    b = counters(dev, other.cuda_stream)
    assert b not in (0, a) and counters(dev, other.cuda_stream) == b


@pytest.mark.parametrize("case", list(launch_cases.CASES))
def test_launch_sequence_is_the_recorded_one(case):
    _need_gpu()
    want = launch_cases.fixture()[case]
    got = launch_cases.record(case)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (case, i, g, w)     # the first call that differs
    assert want and got == want
