"""tools/knobs.py against the package: every switch names a module constant that exists, and a retired switch in the
environment is refused.  No GPU and no built library needed (importing the package loads none)."""
import importlib
import importlib.util
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = os.path.join(REPO, "tools", "knobs.py")


def _knobs():
    """tools/knobs.py's module-level names with no VITCNN_* variable set (importing it applies the environment)"""
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("VITCNN_")}
    try:
        spec = importlib.util.spec_from_file_location("_knobs_under_test", KNOBS)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    finally:
        os.environ.update(saved)


def test_every_switch_names_a_module_constant():
    knobs = _knobs()
    assert knobs.SWITCHES and knobs.APPLIED == {}
    for env, (mod, attr, parse) in knobs.SWITCHES.items():
        assert hasattr(importlib.import_module("vitcnn_amd." + mod), attr), f"{env}: vitcnn_amd.{mod} has no {attr}"
        assert callable(parse)
    assert not set(knobs.RETIRED) & set(knobs.SWITCHES)


def test_a_retired_switch_is_refused():
    env = {k: v for k, v in os.environ.items() if not k.startswith("VITCNN_")}
    env["VITCNN_SCAN_FUSED"] = "0"
    r = subprocess.run([sys.executable, KNOBS], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "VITCNN_SCAN_FUSED" in r.stderr and "retired switch" in r.stderr, r.stderr
