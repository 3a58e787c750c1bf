"""Host half of the detection metric (no GPU): DetectionEvaluator's accumulate against the plain-loop reference (tests/_ap_ref.py)
and against hand-derived known answers (tests/golden/detection_ap_kats.json); the new ABI symbols are declared."""
import json
import math
import re
from pathlib import Path

import numpy as np
import pytest

import _ap_ref as R

ROOT = Path(__file__).resolve().parent.parent
KATS = json.loads((ROOT / "tests" / "golden" / "detection_ap_kats.json").read_text())["cases"]
TOL = 1e-12          # both sides are host fp64 and do the same few operations per recall point


def same(got, want):
    if want is None or (isinstance(want, float) and math.isnan(want)):
        return isinstance(got, float) and math.isnan(got)
    return abs(got - want) <= TOL


def records_of(images):
    """One batch per image, as the kernel would leave it."""
    return [(im["score"][None].astype(np.float32), np.asarray(im["label"], np.int32)[None], R.pack_bits(im["keep"], im["tp"])[None],
             np.asarray(im["order"], np.int32)[None]) for im in images]


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_known_answers(case):
    from boosted_detr_amd import evaluation
    C, thr = case["num_classes"], case["thresholds"]
    images, gt_count = [], np.zeros(C, np.int64)
    for im, want_tp in zip(case["images"], case["expected"]["tp"]):
        r = R.match_image(np.asarray(im["score"], np.float32), im["label"], np.asarray(im["box"], np.float32), im["gt_label"],
                          np.asarray(im["gt_box"], np.float32), im["num_objects"], thr, case["max_dets"], C)
        assert r["tp"].astype(int).tolist() == want_tp                     # the reference's matching gives the hand-derived TPs
        r.update(score=np.asarray(im["score"], np.float32), label=np.asarray(im["label"]))
        gt_count += r["gt_count"]
        images.append(r)
    assert gt_count.tolist() == case["expected"]["gt_count"]
    ref = R.accumulate(images, gt_count, thr)
    got = evaluation.accumulate(records_of(images), gt_count, thr)
    for k in ("AP", "AP50", "AP75", "AR"):
        assert same(ref[k], case["expected"][k]), (k, ref[k])
        assert same(got[k], case["expected"][k]), (k, got[k])
    for c, want in enumerate(case["expected"]["per_class_AP"]):
        assert same(float(got["per_class_AP"][c]), want), (c, got["per_class_AP"][c])
    assert got["num_ground_truths"] == int(gt_count.sum())


def random_images(rng, n_images, N, C, T, score_levels=None):
    images = []
    for _ in range(n_images):
        score = rng.random(N, dtype=np.float32) if score_levels is None else rng.choice(score_levels, N).astype(np.float32)
        label = rng.integers(2, C, N)
        order = np.asarray(sorted(range(N), key=lambda n: (-float(score[n]), n)), np.int32)
        keep = rng.random(N) < 0.8
        # a detection is a TP at the loosest thresholds first: monotone rows, as real matching mostly gives, plus a few odd bits
        level = rng.integers(0, T + 1, N)
        tp = (np.arange(T)[:, None] < level[None, :]) & keep[None, :]
        tp ^= (rng.random((T, N)) < 0.05) & keep[None, :]
        images.append({"score": score, "label": label, "order": order, "keep": keep, "tp": tp})
    return images


@pytest.mark.parametrize("seed,levels", [(0, None), (1, [0.25, 0.5, 0.75]), (2, None)])
def test_accumulate_matches_reference(seed, levels):
    """Hand-built score / label / tp_bits / gt_count: several images, duplicated scores, dropped detections, classes without
    ground truth (with and without detections), a class with ground truth and no detection."""
    from boosted_detr_amd import evaluation
    rng = np.random.default_rng(seed)
    C, T, N = 9, 10, 40
    thr = np.linspace(0.5, 0.95, 10)
    images = random_images(rng, 5, N, C - 1, T, levels)          # class C-1 never detected
    gt_count = rng.integers(1, 30, C)
    gt_count[[0, 1, 4]] = 0                                      # class 4: detections, no ground truth
    ref = R.accumulate(images, gt_count, thr)
    ev = evaluation.DetectionEvaluator(C, thr, max_dets=100)     # constructing one needs no GPU
    got = evaluation.accumulate(records_of(images), gt_count, ev.iou_thresholds)
    for k in ("AP", "AP50", "AP75", "AR"):
        assert abs(got[k] - ref[k]) <= TOL, (k, got[k], ref[k])
    assert 0.0 < ref["AP"] < 1.0
    valid = gt_count > 0
    assert np.abs(got["per_class_AP"][valid] - ref["per_class_AP"][valid]).max() <= TOL
    assert np.isnan(got["per_class_AP"][~valid]).all()
    assert got["per_class_AP"][C - 1] == 0.0                     # ground truth but no detection: AP 0, and it counts


def test_batched_records_equal_per_image_records():
    """Images of one batch are accumulated in row order: [B,N] records give what B records of [1,N] give."""
    from boosted_detr_amd import evaluation
    rng = np.random.default_rng(5)
    images = random_images(rng, 4, 17, 6, 10, [0.5, 0.25])
    gt_count = np.asarray([0, 0, 5, 7, 0, 3])
    thr = np.linspace(0.5, 0.95, 10)
    single = evaluation.accumulate(records_of(images), gt_count, thr)
    recs = records_of(images)
    batched = [tuple(np.concatenate([r[k] for r in recs[:3]]) for k in range(4)), recs[3]]
    both = evaluation.accumulate(batched, gt_count, thr)
    assert all(single[k] == both[k] for k in ("AP", "AP50", "AP75", "AR"))


def test_empty_evaluator_and_bad_arguments():
    from boosted_detr_amd import evaluation
    ev = evaluation.DetectionEvaluator(5)
    assert ev.iou_thresholds.tolist() == np.linspace(0.5, 0.95, 10).tolist() and ev.max_dets == 100
    res = ev.result()
    assert math.isnan(res["AP"]) and res["num_detections"] == 0
    with pytest.raises(ValueError):
        evaluation.DetectionEvaluator(5, np.linspace(0, 1, 16))
    with pytest.raises(ValueError):
        evaluation.DetectionEvaluator(2)


def test_new_symbols_are_declared():
    from boosted_detr_amd import _lib, build, kernels, training
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "bdetr.h").read_text(), flags=re.S)
    for name in ("bdetr_det_postprocess", "bdetr_det_match"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, header)
    assert "detmetric.hip" in build.SOURCES and "-ffp-contract=off" in build.PER_FILE_FLAGS["detmetric.hip"]
    assert callable(kernels.det_postprocess) and callable(kernels.det_match)
    for name in ("predict_raw", "detections", "evaluate"):
        assert callable(getattr(training.Model, name))
    assert issubclass(training.DetectionAP, training.Callback)
    import __graft_entry__
    __graft_entry__.build()
    h = _lib.lib()
    assert h.bdetr_abi_version() == 8 and hasattr(h, "bdetr_det_match") and hasattr(h, "bdetr_det_postprocess")
