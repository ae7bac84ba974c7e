"""Writes tests/golden/launch_trace.json: for every case of tests/launch_cases.py the library calls of one training
forward + backward, in order, as [entry point, [its non-pointer arguments]] (helpers.launch_trace).  It needs a GPU and
the built library, and only the tests' helpers besides: run it from the commit whose launch sequence is to be pinned
(DESIGN.md section 24 names the commit that produced the committed file).
usage: python tests/golden/gen_launch_trace.py [output path]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "vit-cnn_amd"), os.path.join(REPO, "tests"), REPO]

import launch_cases  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else launch_cases.FIXTURE
    traces = {name: launch_cases.record(name) for name in launch_cases.CASES}
    with open(out, "w") as f:   # one call per line: a changed launch is one changed line of the diff
        f.write("{\n" + ",\n".join(
            json.dumps(name) + ": [\n" + ",\n".join(json.dumps(row) for row in rows) + "\n]"
            for name, rows in traces.items()) + "\n}\n")
    for name, rows in traces.items():
        print(f"{name}: {len(rows)} calls")


if __name__ == "__main__":
    main()
