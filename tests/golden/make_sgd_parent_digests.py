"""Digests of the fused SGD entry point (bdetr_sgd_nesterov_clipnorm) on the seeded synthetic tensors of tests/_adamw_ref.py: three
steps, SHA-256 of all weights, all velocities and the per-tensor norms after each.  Recorded ONCE on an MI355X from the build of the
commit BEFORE sqnorm_kernel took its table stride as an argument (the AdamW pull request); tests/test_adamw_gpu.py requires the
current build to reproduce them bit for bit.  The slab reduction is fixed-order, so the digests are reproducible: this script runs
the three steps twice and refuses to write when the two runs disagree.

Usage (on the GPU box): python tests/golden/make_sgd_parent_digests.py [output.json]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import _adamw_ref as R  # noqa: E402

a, b = R.sgd_digests(), R.sgd_digests()
assert a == b, ("two runs of the same build disagree", a, b)
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sgd_parent_digests.json")
with open(path, "w") as f:
    json.dump(a, f, indent=1)
    f.write("\n")
print("wrote", path, json.dumps(a))
