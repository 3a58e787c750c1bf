"""Digests of whole training steps (tests/_step_digests.py: eight eager steps, the same through the captured step, three overflowing
steps redone by the range guard) recorded from the commit BEFORE training.Model's range guard and side-stream tuning became objects
of their own; tests/test_step_digests_gpu.py requires the current tree to reproduce them bit for bit.

The legs run in deterministic mode (kernels.set_deterministic), so they are reproducible: this script runs them twice, in two fresh
processes, and refuses to write unless both agree leg by leg.  The one exception is the redo leg's hashes: the attempts that
overflow compute on out-of-range values, so a hash of that leg that differs between the two processes is left out and named under
"redo_hashes_left_out"; its integer counters must agree regardless.

Usage (on the GPU box, at the parent commit): python tests/golden/make_step_parent_digests.py <parent commit hash> [output.json]"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]


def one_run() -> None:
    import boosted_detr_amd
    boosted_detr_amd.enable_graph_replay()      # as tests/conftest.py does, before HIP initialises
    import torch
    import _step_digests
    print("STEP_DIGESTS " + json.dumps({"rocm": torch.version.hip, **_step_digests.step_digests()}), flush=True)


def main() -> None:
    commit = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "step_parent_digests.json")
    runs = []
    for _ in range(2):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one-run"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        runs.append(json.loads(next(l for l in r.stdout.splitlines() if l.startswith("STEP_DIGESTS ")).split(" ", 1)[1]))
    a, b = runs
    for leg in ("rocm", "inputs", "eager", "graph"):
        assert a[leg] == b[leg], (f"two processes of the same build disagree on '{leg}'", a[leg], b[leg])
    left_out = []
    for k in ("losses", "weights"):
        if a["redo"][k] != b["redo"][k]:
            left_out.append(k)
            del a["redo"][k], b["redo"][k]
    assert a["redo"] == b["redo"], ("two processes of the same build disagree on the redo leg's counters", a["redo"], b["redo"])
    out = {"parent_commit": commit, **a, "redo_hashes_left_out": left_out}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path, json.dumps(out))


if __name__ == "__main__":
    one_run() if sys.argv[1:] == ["--one-run"] else main()
