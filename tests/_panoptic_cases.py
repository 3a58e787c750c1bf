"""Hand-worked panoptic-quality cases, shared by tests/test_panoptic_quality_cpu.py (the reference and the evaluator's host half)
and tests/test_panoptic_quality_gpu.py (the same cases through bdetr_mask_inter and bdetr_panoptic_match).

An image is a 4 x 10 strip of 40 pixels numbered p = 10 y + x; a segment is a range of pixel numbers.  N = 3 queries, M = 3
ground-truth rows, C = 6 classes.  Every case states what it expects: the states, tp / fp / fn summed over the classes and
PQ / SQ / RQ, worked out by hand in the comments."""
import numpy as np

H, W, N, M, C = 4, 10, 3, 3, 6


def _strip(lo, hi):
    m = np.zeros(H * W, bool)
    m[lo:hi] = True
    return m.reshape(H, W)


def _case(pred, gt, min_area=1, **want):
    """pred: [(label, lo, hi)] per query (disjoint ranges); gt: [(label, crowd, lo, hi)] per row (disjoint ranges)."""
    ids = np.full((H, W), -1, np.int64)
    for n, (_, lo, hi) in enumerate(pred):
        ids[_strip(lo, hi)] = n
    masks = np.zeros((M, H, W), bool)
    for m, (_, _, lo, hi) in enumerate(gt):
        masks[m] = _strip(lo, hi)
    return {"pred_ids": ids, "pred_label": np.asarray([p[0] for p in pred] + [2] * (N - len(pred)), np.int32),
            "seg_of": np.asarray(list(range(len(pred))) + [-1] * (N - len(pred)), np.int32),
            "gt_masks": masks, "gt_label": np.asarray([g[0] for g in gt] + [0] * (M - len(gt)), np.int32),
            "gt_crowd": np.asarray([g[1] for g in gt] + [0] * (M - len(gt)), np.uint8), "num_objects": len(gt), "min_area": min_area,
            "want": want}


CASES = {
    # both segments coincide with their ground truths: IoU 1 twice
    "perfect": _case([(2, 0, 20), (3, 20, 40)], [(2, 0, 0, 20), (3, 0, 20, 40)],
                     pred_state=[0, 1, -3], gt_state=[0, 1, -3], tp=2, fp=0, fn=0, PQ=1.0, SQ=1.0, RQ=1.0, classes=2),
    # class 2 only.  Query 0 = pixels 2..11 against row 0 = pixels 0..9: inter 8, its other 2 pixels lie on row 1 (void 0),
    # union 10 + 10 - 8 = 12, IoU 2/3 -> TP.  Query 1 = pixels 12..19 inside row 1 = pixels 10..29: inter 8, union 8 + 20 - 8 = 20,
    # 16 > 20 fails -> FP (nothing of it is void).  Row 1 is matched by nobody -> FN.  SQ = 2/3, RQ = 1 / (1 + 1/2 + 1/2) = 1/2, PQ = 1/3
    "tp_fp_fn": _case([(2, 2, 12), (2, 12, 20)], [(2, 0, 0, 10), (2, 0, 10, 30)],
                      pred_state=[0, -1, -3], gt_state=[0, -1, -3], match_inter=[8, 0, 0], match_union=[12, 0, 0], tp=1, fp=1, fn=1,
                      PQ=(2.0 / 3.0) / 2.0, SQ=2.0 / 3.0, RQ=0.5, classes=1),
    # query 0 (class 2) = pixels 0..9; the only ground truth is of class 3 on pixels 0..3: no match, 6 of its 10 pixels are void,
    # 12 > 10 -> excused.  The ground truth is a FN of class 3: the one scored class has PQ = SQ = RQ = 0
    "mostly_void": _case([(2, 0, 10)], [(3, 0, 0, 4)], pred_state=[-2, -3, -3], gt_state=[-1, -3, -3], tp=0, fp=0, fn=1,
                         PQ=0.0, SQ=0.0, RQ=0.0, classes=1),
    # query 0 (class 2) = pixels 0..9 on a class-2 crowd region = pixels 0..7: crowd 8 + void 2 = 10, 20 > 10 -> excused; nothing scored
    "same_class_crowd": _case([(2, 0, 10)], [(2, 1, 0, 8)], pred_state=[-2, -3, -3], gt_state=[-2, -3, -3], tp=0, fp=0, fn=0,
                              PQ=0.0, SQ=0.0, RQ=0.0, classes=0),
    # the same on a class-3 crowd region: only the 2 void pixels count, 4 > 10 fails -> FP of class 2
    "other_class_crowd": _case([(2, 0, 10)], [(3, 1, 0, 8)], pred_state=[-1, -3, -3], gt_state=[-2, -3, -3], tp=0, fp=1, fn=0,
                               PQ=0.0, SQ=0.0, RQ=0.0, classes=1),
    # query 0 (class 2) = pixels 0..5, row 0 (class 2) = pixels 2..7, row 1 (class 3) = pixels 0..1: inter 4, void 0,
    # union 6 + 6 - 4 = 8, 2 * 4 = 8 is not > 8: IoU exactly 1/2 is no match.  FP of class 2, FN of class 2, FN of class 3
    "iou_exactly_half": _case([(2, 0, 6)], [(2, 0, 2, 8), (3, 0, 0, 2)], pred_state=[-1, -3, -3], gt_state=[-1, -1, -3], tp=0, fp=1, fn=2,
                              PQ=0.0, SQ=0.0, RQ=0.0, classes=2),
    # min_area = 5.  Query 0 = 4 pixels on its own ground truth: below min_area, so no segment - neither matched nor FP - and the
    # ground truth is a FN.  Query 1 = exactly 5 pixels on its own ground truth: a TP at IoU 1
    "min_area": _case([(2, 0, 4), (3, 10, 15)], [(2, 0, 0, 4), (3, 0, 10, 15)], min_area=5,
                      pred_state=[-3, 1, -3], gt_state=[-1, 1, -3], match_inter=[0, 5, 0], match_union=[0, 5, 0], tp=1, fp=0, fn=1,
                      PQ=0.5, SQ=0.5, RQ=0.5, classes=2),
}
