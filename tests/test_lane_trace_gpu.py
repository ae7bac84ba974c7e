"""The ViT-CNN step's lane DAG is the recorded one (tests/golden/vitcnn_lane_trace.json): per case of tests/
lane_cases.py the same library calls with the same non-pointer arguments, on the same lanes, behind the same calls."""
import pytest
import torch

import lane_cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(lane_cases.CASES))
def test_vitcnn_lane_dag_is_the_recorded_one(name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    want, got = lane_cases.fixture()[name], lane_cases.record(name)
    for i, (w, g) in enumerate(zip(want, got)):
        assert g == w, f"{name}: call {i} is {g}, recorded {w}"
    assert len(got) == len(want), f"{name}: {len(got)} calls, recorded {len(want)}"
