"""Whole training steps against digests recorded from the commit before training.Model's range guard and side-stream tuning became
objects of their own (tests/golden/step_parent_digests.json, written by tests/golden/make_step_parent_digests.py): that change moved
host code only, so in deterministic mode every loss and every weight must come out the same to the last bit - eagerly, through the
captured step, and through a range-guard redo with its counter rollback."""
import json
import os

import pytest

import _step_digests

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_training_steps_reproduce_the_parent_commits_digests(cuda):
    import torch
    with open(os.path.join(ROOT, "tests", "golden", "step_parent_digests.json")) as f:
        want = json.load(f)
    got = _step_digests.step_digests()
    assert got["inputs"] == want["inputs"], "the seeded inputs differ: the digests below would say nothing about the step"
    where = f"(digests recorded at {want['parent_commit'][:7]} under ROCm {want['rocm']}; this is ROCm {torch.version.hip})"
    for leg in ("eager", "graph"):
        assert got[leg]["losses"] == want[leg]["losses"], (leg, [i for i, (a, b) in enumerate(zip(got[leg]["losses"], want[leg]["losses"])) if a != b], where)
        assert got[leg]["weights"] == want[leg]["weights"], (leg, where)
    assert got["graph"] == got["eager"]                      # (what test_graph_replayed_steps_equal_eager_steps holds within one process)
    assert want["redo"]["range_redos"] == 1 and want["redo"]["range_skipped"] == 3 and want["redo"]["steps_done"] == 3 and want["redo"]["iterations"] == 3
    for k, v in want["redo"].items():                        # hashes the parent did not reproduce across two processes are not in the file
        assert got["redo"][k] == v, ("redo", k, got["redo"][k], v, where)
