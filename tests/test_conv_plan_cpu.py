"""The convolution launch plans (csrc/igemm.hip, csrc/sgemm.hip) answer the size queries exactly as the commit before them did
(tests/golden/conv_plan_parent.json, written by tests/golden/make_conv_plan_parent.py), and a forced tile without an instantiation
is sized for the tile that launches.  Host code only: no GPU."""
import json
import os

import pytest

import _conv_plan

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_parent.json")) as f:
    PARENT = json.load(f)


def _compare(setting: str, want: dict):
    assert [tuple(g) for g in PARENT["geometries"]] == _conv_plan.geometries() and tuple(PARENT["queries"]) == _conv_plan.QUERIES
    got = _conv_plan.child_table(setting)
    assert sorted(got) == sorted(want)
    diff = [(policy, PARENT["geometries"][i], dict(zip(_conv_plan.QUERIES, zip(w, g))))
            for policy in want for i, (w, g) in enumerate(zip(want[policy], got[policy])) if w != g]
    assert not diff, f"{len(diff)} rows differ (policy, geometry, query: (parent, now)); first: {diff[:3]}"


@pytest.mark.parametrize("setting", ["", "BDETR_TILE=128x128", "BDETR_STILE=128x64", "BDETR_HCONV=0"])
def test_plans_answer_as_the_parent_did(setting):
    _compare(setting, PARENT["tables"][setting])


def test_forced_tile_without_an_instantiation_is_sized_for_the_tile_that_launches():
    """BDETR_TILE=256x64 has no kernel; every launch runs 64x64 then, and the partial-statistics rows and split-K factors must be
    that tile's (the parent sized them for 256x64: a quarter of the rows the epilogue writes)."""
    _compare("BDETR_TILE=256x64", PARENT["tables"]["BDETR_TILE=64x64"])
