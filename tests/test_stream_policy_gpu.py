"""BDETR_STREAM_POLICY (csrc/stream.h): the non-temporal hint on stream-once operands changes no value.

The library reads the switch once per process, so every policy runs in a fresh child (tests/_stream_policy_child.py), once per
module: policy 0 (every access default - the code paths the kernels had before the switch) against policy 63 (every operand
class on).  Per kernel case the SHA-256 of everything the case produced must be equal, and the policy-on child's guard arena
(tests/_guard.py) must have found nothing; three deterministic training steps of the toy model must give bit-identical losses
and weights."""
import json
import os
import subprocess
import sys

import pytest

import _stream_policy_child as child

pytestmark = pytest.mark.gpu

OFF, ON = 0, 63


def _run_child(mode, policy):
    env = dict(os.environ, BDETR_STREAM_POLICY=str(policy))
    p = subprocess.run([sys.executable, os.path.join(child.HERE, "_stream_policy_child.py"), mode], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, "child %s under policy %d failed:\n%s\n%s" % (mode, policy, p.stdout[-2000:], p.stderr[-4000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith(child.MARK)]
    assert len(line) == 1, p.stdout[-2000:]
    out = json.loads(line[0][len(child.MARK):])
    assert out["policy"] == policy, (out["policy"], policy)          # the library saw the switch
    return out


@pytest.fixture(scope="module")
def kernel_runs(cuda):
    return {p: _run_child("kernels", p) for p in (OFF, ON)}


@pytest.fixture(scope="module")
def toy_runs(cuda):
    return {p: _run_child("toy", p) for p in (OFF, ON)}


def test_the_child_ran_every_case(kernel_runs):
    for p in (OFF, ON):
        assert sorted(kernel_runs[p]["cases"]) == sorted(child.CASES)


@pytest.mark.parametrize("name", child.CASES)
def test_kernel_results_are_bit_identical_off_and_on(kernel_runs, name):
    off, on = kernel_runs[OFF]["cases"][name], kernel_runs[ON]["cases"][name]
    assert off["digest"] == on["digest"], name


@pytest.mark.parametrize("name", child.CASES)
def test_guard_arena_is_clean_with_the_policy_on(kernel_runs, name):
    assert kernel_runs[ON]["cases"][name]["guard"] is None, kernel_runs[ON]["cases"][name]["guard"]
    assert kernel_runs[OFF]["cases"][name]["guard"] is None, kernel_runs[OFF]["cases"][name]["guard"]


def test_toy_model_steps_are_bit_identical_off_and_on(toy_runs):
    off, on = toy_runs[OFF], toy_runs[ON]
    assert len(off["losses"]) == 3 and all(float.fromhex(x) == float.fromhex(x) for x in off["losses"])       # three finite-or-inf, non-NaN losses
    assert off["losses"] == on["losses"], (off["losses"], on["losses"])
    assert len(off["weights"]) > 50 and sorted(off["weights"]) == sorted(on["weights"])
    bad = [k for k in off["weights"] if off["weights"][k] != on["weights"][k]]
    assert not bad, bad[:5]
