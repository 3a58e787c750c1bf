"""Host half of the mask metric (no GPU): the plain-loop reference (tests/_mask_ap_ref.py) against hand-derived known answers
(tests/golden/mask_ap_kats.json, written by tests/golden/make_mask_ap_kats.py), MaskEvaluator's host path against the reference,
the new ABI symbols, and the argument checks of the Python layers."""
import json
import math
import re
from pathlib import Path

import numpy as np
import pytest

import _mask_ap_ref as R

ROOT = Path(__file__).resolve().parent.parent
KATS = json.loads((ROOT / "tests" / "golden" / "mask_ap_kats.json").read_text())["cases"]
TOL = 1e-12          # a precision of "1" is 1 / (1 + eps) in COCOeval's accumulate; hand-derived values are met to this, not bit for bit


def same(got, want):
    if want is None or (isinstance(want, float) and math.isnan(want)):
        return isinstance(got, float) and math.isnan(got)
    return abs(got - want) <= TOL


def records_of(images):
    """One batch per image, as the kernels would leave it."""
    return [(im["score"][None].astype(np.float32), np.asarray(im["label"], np.int32)[None], R.pack_bits(im["keep"], im["tp"])[None],
             np.asarray(im["order"], np.int32)[None]) for im in images]


def kat_images(case):
    """The reference's per-image results for a known-answer case, masks binarised the way the product does (logits at 0, targets
    at 0.5)."""
    images, gt_count = [], np.zeros(case["num_classes"], np.int64)
    for im in case["images"]:
        logits = np.where(np.asarray(im["mask"], bool), 1.0, -1.0).astype(np.float32).reshape(len(im["score"]), -1)
        targets = np.asarray(im["gt_mask"], np.float32).reshape(len(im["gt_label"]), -1)
        r = R.match_image(np.asarray(im["score"], np.float32), im["label"], R.binarize(logits, 0.0), im["gt_label"], R.binarize(targets, 0.5),
                          im["num_objects"], case["thresholds"], case["max_dets"], case["num_classes"])
        r.update(score=np.asarray(im["score"], np.float32), label=np.asarray(im["label"]))
        gt_count += r["gt_count"]
        images.append(r)
    return images, gt_count


def test_the_fixture_is_what_its_generator_writes():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_mask_ap_kats", ROOT / "tests" / "golden" / "make_mask_ap_kats.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert json.loads(json.dumps(mod.CASES)) == KATS
    names = [c["name"] for c in KATS]
    assert len(names) == len(set(names)) >= 5


def test_reference_iou_basics():
    d = np.zeros(8, bool)
    assert R.mask_iou(d, d) == 0.0                                                   # empty union: 0, not NaN
    a, b, c = np.isin(np.arange(8), [0, 1, 2]), np.isin(np.arange(8), [0, 1, 3]), np.isin(np.arange(8), [0, 1, 2, 4, 5, 6])
    assert R.mask_iou(a, b) == R.mask_iou(a, c) == 0.5                               # 2/4 and 3/6: the same double
    assert R.mask_iou(a, np.isin(np.arange(8), [0, 1, 2, 3, 4])) == 0.6 < 0.6000000000000001
    x = np.asarray([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, 0.5], np.float32)
    assert R.binarize(x, 0.0).tolist() == [False, False, False, True, False, True, True]
    assert R.binarize(x, 0.5).tolist() == [False, False, False, True, False, False, False]
    words = R.pack_words(np.isin(np.arange(70), [0, 63, 64, 69]))
    assert words.dtype == np.uint64 and words.tolist() == [(1 << 63) | 1, (1 << 5) | 1]


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_known_answers(case):
    from boosted_detr_amd import evaluation
    images, gt_count = kat_images(case)
    exp = case["expected"]
    assert [im["tp"].astype(int).tolist() for im in images] == exp["tp"]             # the reference's matching gives the hand-derived TPs
    assert [im["matched_gt"].tolist() for im in images] == exp["matched_gt"]
    assert gt_count.tolist() == exp["gt_count"]
    ref = R.accumulate(images, gt_count, case["thresholds"])
    ev = evaluation.MaskEvaluator(case["num_classes"], case["thresholds"], case["max_dets"])      # constructing one needs no GPU
    got = ev.result_from(records_of(images), gt_count)
    for k in ("AP", "AP50", "AP75", "AR"):
        assert same(ref[k], exp[k]), (k, ref[k])
        assert same(got[k], exp[k]), (k, got[k])
    if case["name"] == "perfect_masks":
        assert abs(got["AP"] - 1.0) <= TOL and 1.0 in case["thresholds"]
    if case["name"] == "three_fifths_misses_linspace_0_6":
        assert case["thresholds"][2] == 0.6000000000000001 > 0.6                       # the JSON round trip kept the last bit


def coarse_images(seed, n_images=4, N=24, M=9, C=6, side=6):
    """Masks are unions of two rectangles on a side x side grid, scores come from four levels: ties everywhere."""
    rng = np.random.default_rng(seed)

    def rects(n):
        out = np.zeros((n, side, side), bool)
        for i in range(n):
            for _ in range(2):
                y0, x0 = rng.integers(0, side - 1, 2)
                out[i, y0:y0 + rng.integers(1, 4), x0:x0 + rng.integers(1, 4)] = True
        return out.reshape(n, -1)
    batches = []
    for _ in range(n_images):
        gt_mask, gt_label = rects(M), rng.integers(2, C, M).astype(np.int32)
        src = rng.integers(0, M, N)
        mask = np.where(rng.random(N)[:, None] < 0.5, gt_mask[src], rects(N))
        batches.append({"score": rng.choice([0.2, 0.4, 0.6, 0.8], (1, N)).astype(np.float32), "label": gt_label[src][None], "mask": mask[None],
                        "gt_label": gt_label[None], "gt_mask": gt_mask[None], "num_objects": np.asarray([rng.integers(0, M + 1)])})
    return batches


@pytest.mark.parametrize("seed", [0, 1])
def test_mask_evaluator_host_path_matches_reference(seed):
    """Records built from the reference's per-image matches, through MaskEvaluator.result_from: the reference's metrics.  Both sides
    are host fp64 and add the same few hundred samples in different orders; the bar is test_detection_eval_cpu's for that (1e-12)."""
    from boosted_detr_amd import evaluation
    C = 6
    thr = np.linspace(0.5, 0.95, 10)
    ref, images = R.evaluate(coarse_images(seed), thr, 5, C)
    gt_count = sum(im["gt_count"] for im in images)
    ev = evaluation.MaskEvaluator(C, max_dets=5)
    assert ev.iou_thresholds.tolist() == thr.tolist()
    got = ev.result_from(records_of(images), gt_count)
    for k in ("AP", "AP50", "AP75", "AR"):
        assert abs(got[k] - ref[k]) <= TOL, (k, got[k], ref[k])
    assert 0.0 < ref["AP"] < ref["AP50"] < 1.0
    valid = gt_count > 0
    assert np.abs(got["per_class_AP"][valid] - ref["per_class_AP"][valid]).max() <= TOL
    assert not all(im["keep"].all() for im in images)                                # max_dets = 5 truncates
    # several evaluators, one host copy: nothing kept means nothing to copy, and the results are the empty ones
    box, mask = evaluation.DetectionEvaluator(C), evaluation.MaskEvaluator(C)
    empty = evaluation.results([box, mask])
    assert len(empty) == 2 and all(math.isnan(r["AP"]) and r["num_detections"] == 0 for r in empty)


def test_new_symbols_are_declared_and_exported():
    import boosted_detr_amd
    from boosted_detr_amd import _lib, build, evaluation, kernels, training
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "bdetr.h").read_text(), flags=re.S)
    for name in ("bdetr_mask_binarize", "bdetr_mask_match"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, header)
    assert "maskmetric.hip" in build.SOURCES and "-ffp-contract=off" in build.PER_FILE_FLAGS["maskmetric.hip"]
    assert callable(kernels.mask_binarize) and callable(kernels.mask_match)
    assert issubclass(evaluation.MaskEvaluator, evaluation.DetectionEvaluator) and boosted_detr_amd.MaskEvaluator is evaluation.MaskEvaluator
    assert callable(training.Model.segmentations)
    import __graft_entry__
    __graft_entry__.build()
    h = _lib.lib()
    assert h.bdetr_abi_version() == 8 and hasattr(h, "bdetr_mask_binarize") and hasattr(h, "bdetr_mask_match")


def test_wrapper_argument_validation():
    """Dtypes and shapes are checked by name before anything is launched (so this needs no GPU)."""
    import torch
    from boosted_detr_amd import _lib, evaluation
    from boosted_detr_amd import kernels as K
    with pytest.raises(_lib.BdetrError, match="x must be a torch.float32"):
        K.mask_binarize(torch.zeros(2, 5, dtype=torch.float64), 0.0)
    with pytest.raises(_lib.BdetrError, match="at least one element"):
        K.mask_binarize(torch.zeros(2, 0), 0.0)
    B, N, M, W, C = 2, 5, 3, 2, 4
    good = dict(score=torch.zeros(B, N), label=torch.zeros(B, N, dtype=torch.int32), det_bits=torch.zeros(B, N, W, dtype=torch.int64),
                det_area=torch.zeros(B, N, dtype=torch.int32), gt_label=torch.zeros(B, M, dtype=torch.int32),
                gt_bits=torch.zeros(B, M, W, dtype=torch.int64), gt_area=torch.zeros(B, M, dtype=torch.int32),
                num_objects=torch.zeros(B, dtype=torch.int32), thresholds=[0.5], num_classes=C, max_dets=100,
                gt_count=torch.zeros(C, dtype=torch.int32))
    for name, bad, msg in [("det_bits", torch.zeros(B, N, W, dtype=torch.int32), "det_bits must be a torch.int64"),
                           ("gt_bits", torch.zeros(B, M, W, dtype=torch.float32), "gt_bits must be a torch.int64"),
                           ("det_area", torch.zeros(B, N, dtype=torch.int64), "det_area must be a torch.int32"),
                           ("score", torch.zeros(B, N, dtype=torch.float64), "score must be a torch.float32"),
                           ("gt_bits", torch.zeros(B, M, W + 1, dtype=torch.int64), "shapes disagree"),
                           ("det_area", torch.zeros(B, N + 1, dtype=torch.int32), "shapes disagree"),
                           ("gt_area", torch.zeros(B + 1, M, dtype=torch.int32), "shapes disagree"),
                           ("det_bits", torch.zeros(B, N, dtype=torch.int64), "shapes disagree"),
                           ("gt_count", torch.zeros(C + 1, dtype=torch.int32), "shapes disagree")]:
        with pytest.raises(_lib.BdetrError, match=msg):
            K.mask_match(**dict(good, **{name: bad}))
    with pytest.raises(_lib.BdetrError, match="HBM"):
        K.mask_match(**good)                                                         # well-formed, but on the host: no CPU path
    ev = evaluation.MaskEvaluator(C)
    with pytest.raises(ValueError, match="classes"):
        ev.update(torch.zeros(B, N, C + 1), torch.zeros(B, N, 9), torch.zeros(B, M, dtype=torch.int32), torch.zeros(B, M, 9), torch.zeros(B))
    with pytest.raises(ValueError, match="one pixel count"):
        ev.update(torch.zeros(B, N, C), torch.zeros(B, N, 9), torch.zeros(B, M, dtype=torch.int32), torch.zeros(B, M, 3, 4), torch.zeros(B))
    with pytest.raises(ValueError):
        evaluation.MaskEvaluator(C, np.linspace(0, 1, 16))


def test_iou_types_validation():
    """Raised before a batch is looked at (the iterables here would fail if they were).  Building a model needs a GPU, so the models
    here are bare instances with just what the check reads; test_mask_eval_gpu.py repeats this on built models."""
    from boosted_detr_amd.boosted_model import BoostedDETR
    from boosted_detr_amd.model import DETR
    from boosted_detr_amd.training import DetectionAP, Model

    def never():
        raise AssertionError("a batch was requested")
        yield
    plain = object.__new__(DETR)
    plain.__dict__["PanopticAttention"] = None               # what DETR() without with_panoptic_head leaves
    for bad in (("bbox", "keypoints"), "mask", (), ("segm", "Bbox")):
        with pytest.raises(ValueError, match="iou_types"):
            plain.evaluate(never(), iou_types=bad)
        with pytest.raises(ValueError, match="iou_types"):
            DetectionAP([], iou_types=bad)
    assert Model._check_iou_types(["segm", "bbox"]) == ("bbox", "segm") and Model._check_iou_types("segm") == ("segm",)
    with pytest.raises(RuntimeError, match="with_panoptic_head=True") as no_head:
        plain.evaluate(never(), iou_types=("segm",))
    with pytest.raises(RuntimeError) as from_masks:
        plain.panoptic_masks()
    assert str(no_head.value) == str(from_masks.value)                               # the error panoptic_masks() raises
    with pytest.raises(RuntimeError, match="with_panoptic_head=True"):
        plain.segmentations({})
    boosted = object.__new__(BoostedDETR)
    with pytest.raises(RuntimeError, match="BoostedDETR has no mask head"):
        boosted.evaluate(never(), iou_types=("segm",))
    with pytest.raises(RuntimeError, match="BoostedDETR has no mask head"):
        boosted.segmentations({})
    assert DetectionAP([], iou_types="segm").iou_types == ("segm",) and DetectionAP([], iou_types=["segm", "bbox"]).iou_types == ("bbox", "segm")
    assert DetectionAP([]).iou_types == ("bbox",)


@pytest.mark.parametrize("over,names", [(dict(N=1025), b"N <= 1024"), (dict(T=16), b"T in [1, 15]"), (dict(C=2), b"C in [3, 65536]"),
                                        (dict(max_dets=0), b"max_dets >= 1"), (dict(N=1024, M=1024, W=9), b"the limit is 65536"),
                                        (dict(N=100, M=100, W=40), b"need 66904 bytes of LDS")])
def test_launcher_refuses_over_limit_shapes_on_the_host(over, names):
    """The size checks come before anything touches the device or the operands, so they answer here too: status -1 and a message
    that names the limit (the GPU test also shows that nothing was launched)."""
    import ctypes
    import __graft_entry__
    __graft_entry__.build()
    from boosted_detr_amd import _lib
    N, M, W, C, T, max_dets = (over.get(k, v) for k, v in (("N", 8), ("M", 4), ("W", 2), ("C", 5), ("T", 3), ("max_dets", 100)))
    never_read = ctypes.addressof((ctypes.c_char * 64)())
    thr = np.linspace(0.5, 0.95, 16)
    st = _lib.lib().bdetr_mask_match(never_read, never_read, never_read, never_read, never_read, never_read, never_read, never_read,
                                     thr.ctypes.data, 1, N, M, W, C, T, max_dets, never_read, never_read, never_read, never_read, None)
    msg = _lib.lib().bdetr_last_error()
    assert st == -1 and b"bdetr_mask_match" in msg and names in msg, msg
