"""Tables of the convolution size queries (tests/_conv_plan.py) recorded from the commit BEFORE the launch plans of csrc/igemm.hip and
csrc/sgemm.hip: one table per setting of the tile switches that tests/test_conv_plan_cpu.py requires the current tree to reproduce,
plus the table of BDETR_TILE=64x64 - the tile every launch falls back to when BDETR_TILE names one without an instantiation, which
is what the queries must then answer for (at the recorded commit they did not).

Needs no GPU.  Usage (in a checkout of the parent commit with its library built, this file and tests/_conv_plan.py copied into it):
python tests/golden/make_conv_plan_parent.py <parent commit hash> [output.json]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _conv_plan  # noqa: E402

SETTINGS = ("", "BDETR_TILE=128x128", "BDETR_STILE=128x64", "BDETR_HCONV=0", "BDETR_TILE=64x64")


def main() -> None:
    commit = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "conv_plan_parent.json")
    out = {"parent_commit": commit, "queries": list(_conv_plan.QUERIES), "geometries": _conv_plan.geometries(),
           "tables": {s: _conv_plan.child_table(s) for s in SETTINGS}}
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
