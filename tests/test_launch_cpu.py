"""vitcnn_amd.launch: the reference CLI (main.py) patched for the MI355X path (VERDICT r2 missing item 2).

The patch is checked on a synthetic main.py carrying the reference's anchor lines in the reference's
order (the reference's own main.py is program text of another project and is not part of this
repository; `patch_main_source` raises on a main.py whose anchors have drifted).
"""
import pytest

SYNTH = """import torch
import sys
from utils import metrics, get_device
from datasets import get_dataset, MultiModalX
from model_utils import get_model, train, test, pretrain
import argparse
filename = './results/trytry.txt'
sys.stdout = open(filename, 'w')
parser = argparse.ArgumentParser()
parser.add_argument("--cuda", type=int, default=-1)
args = parser.parse_args()
CUDA_DEVICE = get_device(args.cuda)
hyperparams = vars(args)
"""


def _check(src):
    from vitcnn_amd.launch import patch_main_source
    out = patch_main_source(src)
    assert "from vitcnn_amd.model_utils import get_model, train, test" in out
    assert "from model_utils import get_model" not in out
    assert "    from model_utils import pretrain" in out
    assert "from vitcnn_amd.metrics import metrics" in out
    assert out.index("from vitcnn_amd.metrics import metrics") > out.index("from utils import")
    assert "'--precision'" in out and "_vc_parallel.init_from_env()" in out
    assert out.index("'--precision'") < out.index("args = parser.parse_args()")
    assert "torch.device('cuda', _VC_LOCAL) if _VC_WORLD > 1 else get_device(args.cuda)" in out
    assert ".rank' + os.environ['RANK']" in out
    compile(out, "main.py", "exec")
    return out


def test_patch_synthetic_main():
    out = _check(SYNTH)
    # the argparse namespace feeds get_model through hyperparams = vars(args) (main.py:311)
    assert "hyperparams = vars(args)" in out
    assert out.index("args = parser.parse_args()") < out.index("hyperparams = vars(args)")
    from vitcnn_amd.launch import patch_main_source
    with pytest.raises(RuntimeError, match="anchor"):
        patch_main_source(SYNTH.replace("args = parser.parse_args()", "args = parser.parse_known_args()[0]"))

