"""What the size queries of the convolution launch plans answer (csrc/igemm.hip, csrc/sgemm.hip: the partial-statistics row counts and
split-K factors Python allocates from before a launch), for a fixed list of geometries under each of the five precision policies.
No GPU is needed: the queries are host code, and without a device the library assumes the MI355X's 256 CUs.

The switches are read once per process, so one process answers for one setting of the environment: run as a script, this module
prints its table as one line `CONV_PLAN <json>`.  tests/golden/make_conv_plan_parent.py records the tables of the commit before
the launch plans; tests/test_conv_plan_cpu.py compares the current tree against them."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

QUERIES = ("bdetr_conv2d_fwd_stat_chunks", "bdetr_conv2d_bwd_weight_splitk", "bdetr_p16_conv2d_fwd_stat_chunks",
           "bdetr_p16_conv2d_bwd_data_stat_chunks", "bdetr_p16_conv2d_bwd_weight_splitk", "bdetr_p16_supported")
POLICIES = ("fp32", "bf16x3", "mixed", "split", "bf16x6")
RESNET50_STAGES = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))


def geometries():
    """(N, H, W, C, K, R, stride, pad) rows: every distinct convolution of the ResNet-50 backbone at 640x640 for N = 2, 16 and 32, then
    the layers around it and the shapes at which the tile rules change."""
    out = []
    for N in (2, 16, 32):
        out.append((N, 640, 640, 4, 64, 7, 2, 3))                      # stem (three channels padded to four)
        size, cin = 160, 64                                             # after the stem's stride and the max pool
        for f, _, s in RESNET50_STAGES:
            out.append((N, size, size, cin, 4 * f, 1, s, 0))           # projection shortcut
            out.append((N, size, size, cin, f, 1, s, 0))               # first unit's c1 (carries the stage's stride)
            size //= s
            out.append((N, size, size, f, f, 3, 1, 1))                 # c2
            out.append((N, size, size, f, 4 * f, 1, 1, 0))             # c3
            out.append((N, size, size, 4 * f, f, 1, 1, 0))             # later units' c1
            cin = 4 * f
    out += [
        (16, 20, 20, 2048, 256, 1, 1, 0),        # the neck's 1x1
        (16, 94, 94, 32, 100, 3, 4, 0),          # the panoptic head's 3x3 stride-4 ConvOut
        (2, 9, 11, 160, 64, 3, 1, 1),            # the two ragged test shapes
        (2, 13, 9, 64, 224, 3, 1, 1),
        (16, 20, 20, 256, 32, 1, 1, 0),          # K <= 32: the 128x32 tile
        (16, 40, 40, 256, 24, 3, 1, 1),
        (16, 40, 40, 512, 200, 1, 1, 0),         # K no multiple of 128
        (16, 40, 40, 128, 192, 3, 1, 1),
    ]
    out = list(dict.fromkeys(out))               # (stage 2's shortcut and c3 are one geometry)
    assert len(out) >= 60
    return out


def table():
    """{policy: [[the six answers] per geometry]} of this process's environment."""
    sys.path.insert(0, ROOT)
    from boosted_detr_amd import _lib
    L = _lib.lib()
    keep = L.bdetr_get_gemm_precision()
    out = {}
    for mode, policy in enumerate(POLICIES):
        assert L.bdetr_set_gemm_precision(mode) == 0
        rows = []
        for N, H, W, C, K, R, stride, pad in geometries():
            OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
            d = _lib.ConvDesc(N, H, W, C, K, R, R, stride, pad, OH, OW)
            rows.append([int(getattr(L, q)(d)) for q in QUERIES])
        out[policy] = rows
    L.bdetr_set_gemm_precision(keep)
    return out


SWITCHES = ("BDETR_TILE", "BDETR_STILE", "BDETR_HCONV", "BDETR_HCONV_TILE", "BDETR_GEMM_PRECISION", "BDETR_WGRAD_1X1_TILE", "BDETR_WGRAD_WANT",
            "BDETR_WGRAD_WANT_3X3", "BDETR_WGRAD_WANT_64", "BDETR_WGRAD_MINSTAGES", "BDETR_LIB")


def child_table(setting: str):
    """The table of a fresh process under `setting` ('' or 'NAME=value'), every other switch unset."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    if setting:
        name, value = setting.split("=", 1)
        env[name] = value
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("CONV_PLAN ")).split(" ", 1)[1])


if __name__ == "__main__":
    print("CONV_PLAN " + json.dumps(table()), flush=True)
