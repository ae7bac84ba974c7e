"""Writes tests/golden/vitcnn_lane_trace.json: for every case of tests/lane_cases.py the ViT-CNN step's lane DAG, one
library call per line as [entry point, [its non-pointer arguments], lane, [the calls it depends on]]
(helpers.LaneRecorder).  It needs a GPU and the built library, and only the tests' helpers besides: run it from the
commit whose program is to be pinned ("Retired program forms", names the commit that produced the committed
file).
usage: python tests/golden/gen_vitcnn_lane_trace.py [output path]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "vit-cnn_amd"), os.path.join(REPO, "tests"), REPO]

import lane_cases  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else lane_cases.FIXTURE
    traces = {name: lane_cases.record(name) for name in lane_cases.CASES}
    with open(out, "w") as f:   # one call per line: a changed launch or edge is one changed line of the diff
        f.write("{\n" + ",\n".join(
            json.dumps(name) + ": [\n" + ",\n".join(json.dumps(row, separators=(",", ":")) for row in rows) + "\n]"
            for name, rows in traces.items()) + "\n}\n")
    for name, rows in traces.items():
        print(f"{name}: {len(rows)} calls on lanes {sorted({r[2] for r in rows})}")


if __name__ == "__main__":
    main()
