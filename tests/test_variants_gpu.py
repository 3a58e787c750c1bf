"""Every selectable variant of the conv/GEMM kernel family, forced by its environment switch and compared with fp64.

The choosers (hconv_plan, sgemm.hip's choose_tile / bwd_data_plan / bwd_weight_plan, igemm.hip's plan_tile, attn_split_enabled) pick a compiled
variant from the problem size and the CU count; the other kernel tests check whatever they pick for the listed shapes.  Here
each variant is FORCED (the switches are read once per process, so every variant runs in a child process,
tests/_variant_child.py) on the geometries where tiled kernels go wrong, and the parent asserts

  * the project's own bars against fp64 references (2e-5 x max|ref| forward, 6e-5 gradients, 1e-4 statistic sums, 1e-5
    fused-vs-two-pass) - asserted in the child by the imported case bodies and once more here from the reported figures;
  * that the guard arena of every case (tests/_guard.py: 0xFF margins around every operand, result and workspace) found nothing;
  * that the forced variant is among the launched (kind, bm, bn) tuples - a forced tile the chooser silently declines fails -
    and, where the admission rule must refuse it, that it is not.

Children run one after another.  Once one has ended on a signal or on its timeout nothing further is started in the session:
the remaining variant tests fail with "not run after a fault in <variant>"."""
import json
import os
import subprocess
import sys

import pytest

import _variant_child as vc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "_variant_child.py")
_FAULT = []            # the variant whose child died; set once


def run_child(variant, env, argv, timeout):
    """One child process under `env`; never a second one after a fault."""
    if _FAULT:
        pytest.fail("not run after a fault in %s" % _FAULT[0], pytrace=False)
    try:
        r = subprocess.run([sys.executable] + argv, env=dict(os.environ, **env), capture_output=True, text=True, timeout=min(timeout, 600), cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        _FAULT.append(variant)
        pytest.fail("%s: child exceeded %d s\n%s" % (variant, timeout, (e.stdout or b"")[-2000:]), pytrace=False)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _FAULT.append(variant)
        pytest.fail("%s: child ended on a signal (return code %d)\n%s\n%s" % (variant, r.returncode, r.stdout[-2000:], r.stderr[-3000:]), pytrace=False)
    return r


def run_cases(variant, env, list_name, timeout):
    """The child's report for one case list: comparisons re-asserted from the figures, {case tuple: set of launched tuples} returned."""
    r = run_child(variant, env, [CHILD, list_name], timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith(vc.MARK)]
    assert r.returncode == 0 and len(lines) == 1, "%s: return code %d\n%s\n%s" % (variant, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    print(variant, lines[0])
    report = json.loads(lines[0][len(vc.MARK):])
    wanted = vc.case_list(list_name)
    assert [tuple(c["case"]) for c in report["cases"]] == [(kind,) + tuple(args) for kind, args, _ in wanted], "the child ran another case list"
    bad = ["%s (%s): %s" % (c["case"], c["what"], c["failed"]) for c in report["cases"] if c["failed"]]
    assert not bad, "%s:\n%s" % (variant, "\n".join(bad))
    unguarded = ["%s (%s): %s" % (c["case"], c["what"], c["guard"]) for c in report["cases"] if c["guard"] is not None]
    assert not unguarded, "%s:\n%s" % (variant, "\n".join(unguarded))
    for c in report["cases"]:
        assert c["errors"], (variant, c["case"], "compared nothing")
        for name, e in c["errors"].items():
            assert e["rel"] <= e["rtol"], (variant, c["case"], name, e)
    return {tuple(c["case"]): {tuple(t) for t in c["tuples"]} for c in report["cases"]}


def kinds(tuples, code):
    return {t for t in tuples if t[0] % 10000 == code}


# Per-child time limits: wall times measured once on an MI355X (process start, HIP initialisation and the fp64 references included) -
# hconv 3.7 s, stile 3.3 s, wgrad 3.0 s, tile 3.2 s, attention 3.0 s -
# times three, rounded up to the next 10 s (a cold process start is not proportional to the work); run_child caps them at 600 s.
# Re-measured with every case inside the guard arena (margin fills, operand snapshots, the margin scan): hconv 3.4 s, stile 3.7 s,
# wgrad 3.1 s, tile 3.2 s, attention 3.1 s - the same limits by the same rule
@pytest.mark.parametrize("tile", sorted(vc.HCONV_TILES))
def test_hconv_forced_tile_geometry_and_fused_sums(cuda, tile):
    """BDETR_HCONV_TILE: W at the halo capacity and one past it, 1-pixel-wide / -high / 1x1 images, many images inside one tile,
    ragged last tiles (rows % BM in {1, BM - 1}), image boundaries inside a tile, one and three channel chunks, several column
    tiles; forward (f16 pairs, with statistics), backward-data (bf16 pairs, plain and accumulate) and the fused
    BatchNorm-backward sums.  One past the cap the 256-row tiles must be refused; 256x128 then falls back to the 128-row halo
    tile (whose own cap admits W = 92), the other two leave the halo kernel altogether."""
    bm, bn, cap = vc.HCONV_TILES[tile]
    launched = run_cases("BDETR_HCONV_TILE=" + tile, {"BDETR_HCONV_TILE": tile}, "hconv:" + tile, 20)
    for (kind, N, H, W, C, K, *_), tuples in launched.items():
        directions = ((True, C, K), (False, K, C)) if kind == "p16" else ((False, K, C),)           # (forward?, reduction channels, GEMM columns J)
        for fwd, cin, J in directions:
            t = vc.hconv_tuple(tile, fwd)
            if vc.hconv_admits(tile, W, cin, J):
                assert t in tuples, ("forced tile not launched", tile, "fwd" if fwd else "bwd", (N, H, W, C, K), sorted(tuples))
            else:
                assert t not in tuples, ("forced tile launched where it must be refused", tile, (N, H, W, C, K), sorted(tuples))
        if W > cap:
            halo = kinds(tuples, 4000)
            if tile == "256128":
                assert halo and all(t[1] == 128 for t in halo), (tile, W, sorted(halo))
            else:
                assert not halo, ("past the halo cap but still on the halo kernel", tile, W, sorted(halo))


@pytest.mark.parametrize("tile", sorted(vc.STILES))
def test_sgemm_forced_tile_fused_epilogues(cuda, tile):
    """BDETR_STILE (with BDETR_HCONV=0 so that the 3x3 product stays on the im2col kernel): the fused BatchNorm-backward sums of the
    3x3 and 1x1 backward-data and the masked accumulate with and without them, on rows % BM != 0 and C % BN != 0."""
    bm, bn = vc.STILES[tile]
    launched = run_cases("BDETR_STILE=" + tile, {"BDETR_STILE": tile, "BDETR_HCONV": "0"}, "stile:" + tile, 20)
    for case, tuples in launched.items():
        dense = case[0] == "masked" or case[6] == 1
        assert (vc.AR_BF16 * 10000 + (0 if dense else 1000), bm, bn * 10 + 2) in tuples, ("forced tile not launched", tile, case, sorted(tuples))
        assert not kinds(tuples, 4000), (case, sorted(tuples))


def test_wide_1x1_weight_gradient_tile(cuda):
    """BDETR_WGRAD_1X1_TILE=128x128: the 1x1 weight gradients (bf16 and f16 x operand, atomic and deterministic split-K) on the tile
    the default rule replaced by 128x64."""
    launched = run_cases("BDETR_WGRAD_1X1_TILE=128x128", {"BDETR_WGRAD_1X1_TILE": "128x128"}, "wgrad", 20)
    hit = 0
    for (kind, N, H, W, C, K, R, stride, pad), tuples in launched.items():
        if K % 128 == 0 and C % 128 == 0:
            # (a strided 1x1 reads x through the patch loader: class 3000)
            assert (vc.AR_BF16 * 10000 + (2000 if stride == 1 else 3000), 128, 1282) in tuples, ((N, H, W, C, K), sorted(tuples))
            hit += 1
    assert hit >= 2


def test_attention_without_the_split_products(cuda):
    """BDETR_ATTN_SPLIT=0: under policy 'split' the attention kernels then run the exact-fp32 MFMA and meet that policy's bars."""
    run_cases("BDETR_ATTN_SPLIT=0", {"BDETR_ATTN_SPLIT": "0"}, "attn", 20)


@pytest.mark.parametrize("tile", ["128x128", "128x64"])
def test_igemm_forced_tile(cuda, tile):
    """BDETR_TILE: the in-kernel-split family on the big tiles at ragged shapes, under the exact-fp32 and the split policy."""
    bm, bn = (int(v) for v in tile.split("x"))
    launched = run_cases("BDETR_TILE=" + tile, {"BDETR_TILE": tile}, "tile", 20)
    ariths = set()
    for case, tuples in launched.items():
        forced = {t for t in tuples if t[1:] == (bm, bn) and t[0] % 10000 < 4000}
        assert forced, ("forced tile not launched", tile, case, sorted(tuples))
        ariths |= {t[0] // 10000 for t in forced}
    assert {0, 1, 2} <= ariths, ariths           # AR_FP32, AR_BF16X3 (gradients), AR_FP16X3 (forward) all ran on it
