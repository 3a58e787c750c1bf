"""Host half of attribute-aware AP (no GPU): the plain-loop reference (tests/_attr_ref.py) against hand-derived F1 values and a
hand-derived image, evaluation.AttributeEvaluator's accumulate against the reference's summary, the reduction to the COCO protocol at
an F1 threshold of 0, every refusal that must come before a launch, and the new ABI symbols."""
import inspect
import math
import re
from pathlib import Path

import numpy as np
import pytest

import _attr_ref as AR
import _coco_ref as R

ROOT = Path(__file__).resolve().parent.parent
SCALARS = ("AP", "AP_IoU50", "AP_IoU75", "AP_F1_50", "AP_F1_75", "AP_small", "AP_medium", "AP_large", "AR_1", "AR_10", "AR_100", "AR_small",
           "AR_medium", "AR_large")


def exactly(got, want):
    return got == want or (math.isnan(got) and math.isnan(want))


def hot(A, *sets):
    """Multi-hot rows [len(sets), A] from sets of attribute indices."""
    x = np.zeros((len(sets), A), np.float32)
    for r, s in enumerate(sets):
        x[r, list(s)] = 1.0
    return x


def f1_of(d, g, empty_f1=1.0, A=70):
    bits, count = AR.attr_pack(hot(A, d, g))
    return AR.f1(bits[0], count[0], bits[1], count[1], empty_f1)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the F1 rule, by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_f1_by_hand():
    assert f1_of({2, 3}, {3, 4}) == 0.5 and AR.passes(*gate_rows({2, 3}, {3, 4}), 0.5, 1.0)             # 2 * 1 / (2 + 2): ON 0.5
    assert f1_of({2, 3, 4, 5}, {3, 4, 5, 69}) == 0.75 and AR.passes(*gate_rows({2, 3, 4, 5}, {3, 4, 5, 69}), 0.75, 1.0)      # 2 * 3 / (4 + 4): ON 0.75
    assert not AR.passes(*gate_rows({2, 3, 4, 5}, {3, 4, 5, 69}), 0.8, 1.0)
    assert f1_of({2}, {2, 3}) == np.float64(2) / np.float64(3) and f1_of({2, 64}, {2, 64}) == 1.0 and f1_of({2}, {3}) == 0.0
    assert f1_of({7}, set()) == 0.0                                  # one side empty: no common attribute
    assert f1_of(set(), set(), 1.0) == 1.0 and f1_of(set(), set(), 0.0) == 0.0
    assert AR.passes(*gate_rows(set(), set()), 0.95, 1.0) and not AR.passes(*gate_rows(set(), set()), 0.5, 0.0)
    assert AR.passes(*gate_rows(set(), set()), 0.0, 0.0)             # a threshold of 0 lets everything through
    assert AR.passes(*gate_rows({2, 3}, {2, 3}), 1.0, 1.0)           # the bound is min(threshold, 1 - 1e-10), as for the IoU
    # <PAD> (0) and <OOV> (1) are never an attribute: a target row with those bits set scores as the one without
    assert f1_of({0, 1, 2, 3}, {3, 4}) == f1_of({2, 3}, {3, 4}) == 0.5 and f1_of({0, 1}, {0}) == f1_of(set(), set()) == 1.0
    bits, count = AR.attr_pack(hot(70, {0, 1, 2, 63, 64, 69}))
    assert bits.dtype == np.uint64 and bits.shape == (1, 2) and count.tolist() == [4]
    assert int(bits[0, 0]) == (1 << 2) | (1 << 63) and int(bits[0, 1]) == (1 << 0) | (1 << 5)
    x = np.asarray([[0.9, 0.9, 0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nan, 0.75]], np.float32)
    bits, count = AR.attr_pack(x)
    assert int(bits[0, 0]) == (1 << 2) | (1 << 5) and count.tolist() == [2]      # >= 0.5; the float below it and NaN are not set


def gate_rows(d, g, A=70):
    bits, count = AR.attr_pack(hot(A, d, g))
    return (None, bits[0], count[0]), (None, bits[1], count[1])


# ---------------------------------------------------------------------------------------------------------------------
# 2. a hand-derived image: the best-IoU ground truth fails the gate, the detection takes the second best, and a later detection takes
#    the one that stayed free
# ---------------------------------------------------------------------------------------------------------------------
def hand_image(f1_thresholds):
    A = 8
    g0, g1 = [0.1, 0.1, 0.4, 0.4], [0.15, 0.1, 0.4, 0.4]            # IoU(g0, g1) = 0.14 / 0.18 = 0.78
    box = np.asarray([g0, g0], np.float32)                           # both detections sit exactly on g0
    return AR.match_image(np.asarray([0.9, 0.8], np.float32), [2, 2], box, hot(A, {2, 3}, {4, 5}), [2, 2], np.asarray([g0, g1], np.float32),
                          hot(A, {4, 5}, {2, 3}), None, None, 2, 100, 100, [0.5], f1_thresholds, 1.0, [[0.0, 1e10]], 100, 3)


def test_hand_derived_redirect():
    per_f, k = hand_image([0.0, 0.5])
    assert k["gate_off"]["matched_gt"][0, 0].tolist() == [0, 1]     # without a gate: d0 takes g0 (IoU 1), d1 what is left
    assert per_f[0]["matched_gt"][0, 0].tolist() == [0, 1]           # an F1 threshold of 0 is no gate
    assert per_f[1]["matched_gt"][0, 0].tolist() == [1, 0]           # F1(d0, g0) = 0: d0 takes g1 (IoU 0.78), d1 the freed g0
    assert per_f[1]["tp"][0, 0].tolist() == [True, True] and k["redirected"] == 2 and k["empty_pairs"] == 0
    assert per_f[1]["gt_count"].tolist() == per_f[0]["gt_count"].tolist() == [[0, 0, 2]]
    # at an IoU threshold the second best does not reach, the gate leaves d0 unmatched instead
    A = 8
    g0, g1 = [0.1, 0.1, 0.4, 0.4], [0.15, 0.1, 0.4, 0.4]
    per_f, _ = AR.match_image(np.asarray([0.9], np.float32), [2], np.asarray([g0], np.float32), hot(A, {2, 3}), [2, 2], np.asarray([g0, g1], np.float32),
                              hot(A, {4, 5}, {2, 3}), None, None, 2, 100, 100, [0.8], [0.5], 1.0, [[0.0, 1e10]], 100, 3)
    assert per_f[0]["matched_gt"][0, 0].tolist() == [-1] and not per_f[0]["tp"].any()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the host accumulate against the reference's summary, on the reference's own match results
# ---------------------------------------------------------------------------------------------------------------------
def batch_of(c, masks=False):
    return {"score": c["score"], "label": c["label"], "det": c["mask" if masks else "box"], "det_attr": c["det_attr"], "gt_label": c["gt_label"],
            "gt": c["gt_mask" if masks else "gt_box"], "gt_attr": c["gt_attr"], "gt_crowd": c["gt_crowd"], "gt_area": c["gt_area"],
            "num_objects": c["num_objects"], "height": c["image_hw"][:, 0], "width": c["image_hw"][:, 1]}


@pytest.fixture(scope="module")
def main_case():
    c = AR.case("B2_N10_M7_A66")
    ref, images, counters = AR.evaluate([batch_of(c)], c["thresholds"], c["f1_thresholds"], 1.0, c["area_ranges"].tolist(), (1, 10, 100), c["C"])
    return c, ref, images, counters


def test_accumulate_matches_reference_exactly(main_case):
    from boosted_detr_amd import evaluation
    c, ref, images, _ = main_case
    ev = evaluation.AttributeEvaluator(c["C"], c["A"])              # constructing one needs no GPU
    assert isinstance(ev, evaluation.CocoEvaluator) and ev.attr_words == 2 and ev.empty_f1 == 1.0 and ev.max_dets == (1, 10, 100)
    assert np.array_equal(ev.f1_thresholds, AR.THR10) and np.array_equal(ev.iou_thresholds, AR.THR10)
    got = ev.result_from(AR.records_of(images, 4), ref["gt_count"])
    assert list(got)[:15] == list(SCALARS) + ["stats"] and len(got["stats"]) == 14
    for i, k in enumerate(SCALARS):
        assert exactly(got[k], ref[k]) and exactly(got["stats"][i], ref["stats"][i]), (k, got[k], ref[k])
    assert exactly(got["AR"], ref["AR"]) and np.array_equal(got["per_class_AP"], ref["per_class_AP"], equal_nan=True)
    assert np.shape(got["AP_table"]) == (10, 10)
    for t in range(10):
        for f in range(10):
            assert exactly(got["AP_table"][t][f], ref["AP_table"][t][f]), (t, f)
    assert got["num_images"] == 2 and np.array_equal(got["gt_count_per_range"], ref["gt_count"]) and got["num_detections"] > 0
    assert 0.0 < ref["AP"] < ref["AP_F1_50"] and ref["AP"] < ref["AP_IoU50"]          # the gate bites, more at the higher thresholds
    empty = evaluation.AttributeMaskEvaluator(5, 9).result()
    assert all(math.isnan(v) for v in empty["stats"]) and len(empty["stats"]) == 14 and empty["num_detections"] == 0


def test_f1_threshold_zero_is_the_coco_protocol(main_case):
    from boosted_detr_amd import evaluation
    c = main_case[0]
    _, images, _ = AR.evaluate([batch_of(c)], c["thresholds"], [0.0], 0.0, c["area_ranges"].tolist(), (1, 10, 100), c["C"])
    plain, plain_images, _ = R.evaluate([{k: v for k, v in batch_of(c).items() if k not in ("det_attr", "gt_attr")}], c["thresholds"],
                                        c["area_ranges"].tolist(), (1, 10, 100), c["C"])
    for im, want in zip(images[0], plain_images):
        assert all(np.array_equal(im[k], want[k]) for k in ("order", "class_rank", "keep", "tp", "ig", "matched_gt", "gt_count"))
    recs = AR.records_of(images, 4)
    got = evaluation.AttributeEvaluator(c["C"], c["A"], f1_thresholds=(0.0,)).result_from(recs, plain["gt_count"])
    coco = evaluation.accumulate_coco([(s, l, cr, tp[0], ig[0], o) for s, l, cr, tp, ig, o in recs], plain["gt_count"], c["thresholds"], (1, 10, 100),
                                      R.COCO_AREA_NAMES)
    for k in ("AP", "AP_small", "AP_medium", "AP_large", "AR_1", "AR_10", "AR_100", "AR_small", "AR_medium", "AR_large"):
        assert exactly(got[k], coco[k]) and exactly(got[k], plain[k]), (k, got[k], coco[k])      # bit for bit
    assert exactly(got["AP_IoU50"], coco["AP50"]) and exactly(got["AP_IoU75"], coco["AP75"]) and math.isnan(got["AP_F1_50"])


def test_gpu_cases_exercise_the_gate():
    """A property of the reference alone: the seeds of the shared cases give redirected detections and empty / empty pairs."""
    for name in list(AR.BOX_SHAPES) + ["mask"]:
        ref = AR.reference(name)
        assert sum(k["redirected"] for _, k in ref) > 0 and sum(k["empty_pairs"] for _, k in ref) > 0, name
    c = AR.case("B2_N10_M7_A66")
    assert c["gt_crowd"].any() and c["gt_area"] is not None and c["num_objects"].tolist() == [7, 5] and c["gt_label"][0, 1] == 0
    assert (AR.case("B1_N70_M70_A296")["gt_label"] == 2).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. refusals: a ValueError, and nothing launched
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_a_launch(monkeypatch):
    import torch
    from boosted_detr_amd import _lib, evaluation, kernels
    from boosted_detr_amd.evaluation import AttributeEvaluator, AttributeMaskEvaluator
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("a refusal reached the library"))
    for bad in (dict(f1_thresholds=[]), dict(f1_thresholds=np.linspace(0, 1, 17)), dict(empty_f1=0.5), dict(iou_thresholds=np.linspace(0, 1, 16))):
        with pytest.raises(ValueError):
            AttributeEvaluator(5, 9, **bad)
    for A in (2, 4097):
        with pytest.raises(ValueError, match="num_attributes"):
            AttributeEvaluator(5, A)
        with pytest.raises(ValueError, match="num_attributes"):
            kernels.attr_pack(torch.zeros(3, A))
    assert AttributeEvaluator(5, 3).attr_words == 1 and AttributeEvaluator(5, 4096, f1_thresholds=np.linspace(0, 1, 16)).attr_words == 64

    # the staging formula of include/bdetr.h, and a batch over 64 KiB
    assert kernels.attr_match_lds_bytes(100, 100, 5) == 36 * 100 + 20 * 100 + 200 + 44 * 200 == 14600
    assert kernels.attr_match_lds_bytes(10, 7, 2) == 36 * 12 + 20 * 8 + 24 + 20 * 20
    assert kernels.attr_match_lds_bytes(10, 7, 2, mask_words=9) == 24 * 12 + 8 * 8 + 24 + 72 * 20 + 20 * 20
    B, N, M, C, A = 1, 100, 100, 5, 4096                               # Wa = 64: 516 bytes a row
    assert kernels.attr_match_lds_bytes(N, M, 64) > 64 * 1024
    ev = AttributeEvaluator(C, A)
    cat_pred, att_pred, box = torch.zeros(B, N, C), torch.zeros(B, N, A), torch.zeros(B, N, 4)
    cat_ids, att_hot, bbox, nobj = torch.zeros(B, M, dtype=torch.int32), torch.zeros(B, M, A), torch.zeros(B, M, 4), torch.zeros(B, dtype=torch.int32)
    with pytest.raises(ValueError, match="bytes of LDS"):
        ev.update(cat_pred, att_pred, box, cat_ids, att_hot, bbox, nobj, image_hw=(64, 64))
    assert ev._kept == [] and ev._gt_count is None
    with pytest.raises(ValueError, match="built for 4096 attributes"):
        ev.update(cat_pred, att_pred[..., :100], box, cat_ids, att_hot, bbox, nobj, image_hw=(64, 64))
    mev = AttributeMaskEvaluator(C, 296)
    with pytest.raises(ValueError, match="bytes of LDS"):               # 32 * 300 + 600 + (8 * 9 + 44) * 600 = 79800 bytes
        mev.update(torch.zeros(B, 300, C), torch.zeros(B, 300, 296), torch.zeros(B, 300, 529), torch.zeros(B, 300, dtype=torch.int32),
                   torch.zeros(B, 300, 296), torch.zeros(B, 300, 529), nobj, image_hw=(64, 64))
    assert mev._kept == [] and mev._gt_count is None
    # the wrappers refuse the same before they look at the device
    z = torch.zeros
    args = dict(score=z(B, N), label=z(B, N, dtype=torch.int32), box_pred=box, det_attr=z(B, N, 2, dtype=torch.int64), det_count=z(B, N, dtype=torch.int32),
                gt_label=cat_ids, gt_box=bbox, gt_attr=z(B, M, 2, dtype=torch.int64), gt_attr_count=z(B, M, dtype=torch.int32),
                gt_crowd=z(B, M, dtype=torch.uint8), gt_area=None, num_objects=nobj, image_hw=z(B, 2, dtype=torch.int32),
                area_ranges=z(1, 2, dtype=torch.float64), thresholds=[0.5], num_classes=C, max_dets=100, gt_count=z(1, C, dtype=torch.int32))
    for gate, match in ((dict(f1_thresholds=[], empty_f1=1.0), "F1 thresholds"), (dict(f1_thresholds=[0.5] * 17, empty_f1=1.0), "F1 thresholds"),
                        (dict(f1_thresholds=[0.5], empty_f1=0.5), "empty_f1")):
        with pytest.raises(ValueError, match=match):
            kernels.det_match_attr(**args, **gate)
    wide = dict(args, det_attr=z(B, N, 64, dtype=torch.int64), gt_attr=z(B, M, 64, dtype=torch.int64))
    with pytest.raises(ValueError, match="bytes of LDS"):
        kernels.det_match_attr(**wide, f1_thresholds=[0.5], empty_f1=1.0)


def test_segm_needs_the_panoptic_head():
    from boosted_detr_amd.boosted_model import BoostedDETR
    from boosted_detr_amd.training import AttributeAP, Model
    model = BoostedDETR.__new__(BoostedDETR)                            # no weights, no device: the refusal comes first
    with pytest.raises(RuntimeError, match="no mask head"):
        model.evaluate_attributes([], iou_types=("bbox", "segm"))
    with pytest.raises(ValueError, match="iou_types"):
        model.evaluate_attributes([], iou_types=("keypoints",))
    with pytest.raises(ValueError, match="iou_types"):
        AttributeAP([], iou_types=())
    p = inspect.signature(Model.evaluate_attributes).parameters
    assert list(p) == ["self", "x", "steps", "iou_types", "evaluator", "mask_evaluator", "iou_thresholds", "f1_thresholds", "empty_f1", "return_dict",
                       "verbose"]
    assert p["iou_types"].default == ("bbox",) and p["empty_f1"].default == 1.0 and p["return_dict"].default is True
    assert callable(Model.attribute_detections) and AttributeAP([], every=2, iou_types="segm").iou_types == ("segm",)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the new symbols
# ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared():
    from boosted_detr_amd import _lib, build, kernels
    full = (ROOT / "include" / "bdetr.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert "K29" in full and "K30" in full and "K31" in full and "fashionpedia-api" in full
    for name in ("bdetr_attr_pack", "bdetr_det_match_attr", "bdetr_mask_match_attr"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, header)
    assert "attrmetric.hip" in build.SOURCES and "-ffp-contract=off" in build.PER_FILE_FLAGS["attrmetric.hip"]
    assert callable(kernels.attr_pack) and callable(kernels.det_match_attr) and callable(kernels.mask_match_attr)
    import __graft_entry__
    __graft_entry__.build()
    h = _lib.lib()
    assert h.bdetr_abi_version() == 8 and all(hasattr(h, n) for n in ("bdetr_attr_pack", "bdetr_det_match_attr", "bdetr_mask_match_attr"))
    # the entries refuse bad sizes without a launch (no GPU is touched)
    assert h.bdetr_attr_pack(1, 1, 2, 1, 1, None) == -1 and b"A in [3, 4096]" in h.bdetr_last_error()
    import ctypes
    f1s = (ctypes.c_double * 16)(*([0.5] * 16))                          # read on the host before the LDS check: a real pointer
    one = [1] * 15 + [ctypes.cast(f1s, ctypes.c_void_p)]
    assert h.bdetr_det_match_attr(*one, 1.0, 1, 4, 4, 3, 1, 1, 17, 1, 1, 1, 1, 1, 1, 1, 1, None) == -1 and b"F in [1, 16]" in h.bdetr_last_error()
    assert h.bdetr_det_match_attr(*one, 0.5, 1, 4, 4, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, None) == -1 and b"empty_f1 0 or 1" in h.bdetr_last_error()
    assert h.bdetr_det_match_attr(*one, 1.0, 1, 4, 4, 3, 65, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, None) == -1 and b"Wa in [1, 64]" in h.bdetr_last_error()
    assert h.bdetr_det_match_attr(*one, 1.0, 1, 100, 100, 3, 64, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, None) == -1 and b"bytes of LDS" in h.bdetr_last_error()
    assert h.bdetr_mask_match_attr(*([1] * 17), one[-1], 1.0, 1, 300, 300, 529, 3, 5, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, None) == -1 \
        and b"bytes of LDS" in h.bdetr_last_error()
