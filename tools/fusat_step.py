"""GPU tool: bench.py's config-5 leg alone -- the FusAtNet B=64 training step as one hipGraph (and its
train-mode forward); prints the leg's JSON.
usage: python tools/fusat_step.py [steps] [--precision {fp32,bf16,bf16_store}]

--precision bf16 / bf16_store (DESIGN.md sections 25, 30) runs the same leg on a model built with that precision:
bench.py's leg builds `FusAtNet(144, 1, 16)`, so the tool hands it a class whose default precision is that one for the
call.  The line is the same; "dtype" names the mode, and since "mfma_frac" stays relative to the fp32 MFMA peak, as in
the fp32 line, the bf16 line says so in "mfma_frac_of".  (The class is looked up on `vitcnn_amd.fusatnet` when the leg runs; if
bench.py ever binds it earlier, the check below fails loudly instead of timing an fp32 model.)"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "vit-cnn_amd"))
import knobs  # noqa: F401,E402  (measurement switches: tools/knobs.py)
import bench  # noqa: E402


def fusat_leg(steps, precision):
    from vitcnn_amd import fusatnet
    if precision == "fp32":
        return bench.fusat_leg(torch.device("cuda", 0), steps, False)[0]
    orig = fusatnet.FusAtNet

    built = []

    class FusAtNetBf16(orig):
        def __init__(self, *args, **kwargs):
            kwargs.setdefault("precision", precision)
            super().__init__(*args, **kwargs)
            built.append(self.precision)

    fusatnet.FusAtNet = FusAtNetBf16
    try:
        out = bench.fusat_leg(torch.device("cuda", 0), steps, False)[0]
    finally:
        fusatnet.FusAtNet = orig
    if built != [precision]:
        raise RuntimeError(f"the leg did not build one {precision} model (built: {built})")
    out["dtype"] = "bf16 3x3-conv operands, fp32 accumulation"
    if precision == "bf16_store":
        out["dtype"] += " (operands stored as bf16)"
    out["mfma_frac_of"] = "fp32 MFMA peak"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=5)
    ap.add_argument("--precision", choices=("fp32", "bf16", "bf16_store"), default="fp32")
    a = ap.parse_args()
    print(json.dumps(fusat_leg(a.steps, a.precision)), flush=True)


if __name__ == "__main__":
    main()
