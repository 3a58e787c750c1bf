"""Writes mask_ap_kats.json: known-answer cases for the mask metric whose results follow by hand.

    python tests/golden/make_mask_ap_kats.py

Nothing is computed here: masks are given as lists of on-pixels on a P-pixel row, and every expected value below is written out
from the derivation in the comment above it.  'tp' and 'matched_gt' are [image][threshold][query]; null stands for NaN (a
threshold that is not among the case's).  A test turns a mask into logits (+1 on, -1 off) or targets (1.0 on, 0.0 off).

How an AP follows from the TPs (COCOeval.accumulate): per class and threshold the detections are walked in descending score;
after each one recall = TP / #gt and precision = TP / (TP + FP + eps), eps = 2^-52; precision is made non-increasing from the right;
each of the 101 recall points 0, 0.01, ..., 1 samples the precision at the first detection whose recall reaches it, or 0 if none
does.  AP is the mean of those samples, AR the final recall.  A precision of 1 is 1 / (1 + eps), 2.2e-16 short of 1: an expected
"1.0" below is met within 1e-12, never bit for bit - that is COCOeval's own eps.
"""
import json
from pathlib import Path


def image(P, dets, gts, num_objects=None):
    """dets: (score, label, on-pixels); gts: (label, on-pixels)."""
    def row(on):
        return [1 if p in on else 0 for p in range(P)]
    return {"score": [d[0] for d in dets], "label": [d[1] for d in dets], "mask": [row(d[2]) for d in dets],
            "gt_label": [g[0] for g in gts], "gt_mask": [row(g[1]) for g in gts], "num_objects": len(gts) if num_objects is None else num_objects}


CASES = []

# One detection {0,1,2} (3 pixels) of class 2 and two ground truths of class 2:
#   g0 = {0,1,3}:         inter {0,1} = 2, union {0,1,2,3} = 4        -> IoU 2/4
#   g1 = {0,1,2,4,5,6}:   inter {0,1,2} = 3, union {0,..,6} \ {3} = 6 -> IoU 3/6
# 2/4 and 3/6 are the same double (0.5), both meet the threshold 0.5, and COCOeval's scan `if iou < best: continue` lets a later
# ground truth with an EQUAL IoU replace an earlier one: the detection takes g1.
# One TP, two ground truths: recall 1/2, precision 1.  The recall points 0 .. 0.5 (51 of 101: linspace(0,1,101)[50] is 0.5
# exactly) sample precision 1, the other 50 sample 0: AP = AP50 = 51/101, AR = 1/2.
CASES.append({"name": "exact_tie_2_4_vs_3_6_larger_index_wins", "num_classes": 3, "thresholds": [0.5], "max_dets": 100,
              "images": [image(8, [(0.9, 2, {0, 1, 2})], [(2, {0, 1, 3}), (2, {0, 1, 2, 4, 5, 6})])],
              "expected": {"tp": [[[1]]], "matched_gt": [[[1]]], "gt_count": [0, 0, 2], "AP": 51 / 101, "AP50": 51 / 101, "AP75": None, "AR": 0.5}})

# The same with the ground truths swapped (g0 is now the 3/6 one, g1 the 2/4 one): still the LARGER index, so which one wins is
# the index's doing and not the mask's.
CASES.append({"name": "exact_tie_swapped_still_larger_index", "num_classes": 3, "thresholds": [0.5], "max_dets": 100,
              "images": [image(8, [(0.9, 2, {0, 1, 2})], [(2, {0, 1, 2, 4, 5, 6}), (2, {0, 1, 3})])],
              "expected": {"tp": [[[1]]], "matched_gt": [[[1]]], "gt_count": [0, 0, 2], "AP": 51 / 101, "AP50": 51 / 101, "AP75": None, "AR": 0.5}})

# Detection {0,1}, ground truth {0,1,2,3}: inter 2, union 4, IoU 2/4 = 0.5 exactly, and 0.5 >= 0.5 matches.  At 0.75 it does not.
# Threshold 0.5: one TP of one ground truth, recall 1, precision 1 at every recall point: AP50 = 1.  Threshold 0.75: one FP,
# recall 0, precision 0: AP75 = 0.  AP = (1 + 0) / 2, AR = (1 + 0) / 2.
CASES.append({"name": "iou_exactly_on_threshold_matches", "num_classes": 3, "thresholds": [0.5, 0.75], "max_dets": 100,
              "images": [image(8, [(0.9, 2, {0, 1})], [(2, {0, 1, 2, 3})])],
              "expected": {"tp": [[[1], [0]]], "matched_gt": [[[0], [-1]]], "gt_count": [0, 0, 1], "AP": 0.5, "AP50": 1.0, "AP75": 0.0, "AR": 0.5}})

# COCO's ten thresholds are np.linspace(0.5, 0.95, 10).  Computed as 0.5 + 2 * 0.05 (NumPy before 2.x) the third one is
# 0.6000000000000001, one ulp ABOVE the double nearest to 0.6; the values are written out here so that the case does not depend
# on the NumPy that runs it.  Detection {0,1,2}, ground truth {0,1,2,3,4}: IoU 3/5 = the double nearest to 0.6, which is below
# that threshold.  So the detection is a TP at 0.5 and 0.55 only (AP 1 there, 0 at the other eight): AP = AR = 2/10, AP50 = 1,
# AP75 = 0.
LINSPACE_THRESHOLDS = [0.5, 0.55, 0.6000000000000001, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]
CASES.append({"name": "three_fifths_misses_linspace_0_6", "num_classes": 3, "thresholds": LINSPACE_THRESHOLDS, "max_dets": 100,
              "images": [image(8, [(0.9, 2, {0, 1, 2})], [(2, {0, 1, 2, 3, 4})])],
              "expected": {"tp": [[[1], [1], [0], [0], [0], [0], [0], [0], [0], [0]]],
                           "matched_gt": [[[0], [0], [-1], [-1], [-1], [-1], [-1], [-1], [-1], [-1]]],
                           "gt_count": [0, 0, 1], "AP": 0.2, "AP50": 1.0, "AP75": 0.0, "AR": 0.2}})

# The counterpart: against the threshold 0.6 itself (the double nearest to it, which is what 3/5 rounds to) the same pair matches.
CASES.append({"name": "three_fifths_meets_0_6", "num_classes": 3, "thresholds": [0.6], "max_dets": 100,
              "images": [image(8, [(0.9, 2, {0, 1, 2})], [(2, {0, 1, 2, 3, 4})])],
              "expected": {"tp": [[[1]]], "matched_gt": [[[0]]], "gt_count": [0, 0, 1], "AP": 1.0, "AP50": None, "AP75": None, "AR": 1.0}})

# An empty prediction against an empty ground truth: the union is empty, the IoU is DEFINED as 0 (not 0/0), below every threshold.
# One FP, one unmatched ground truth: recall 0, precision 0 everywhere.
CASES.append({"name": "empty_against_empty_is_iou_zero", "num_classes": 3, "thresholds": [0.5, 0.75], "max_dets": 100,
              "images": [image(8, [(0.9, 2, set())], [(2, set())])],
              "expected": {"tp": [[[0], [0]]], "matched_gt": [[[-1], [-1]]], "gt_count": [0, 0, 1], "AP": 0.0, "AP50": 0.0, "AP75": 0.0, "AR": 0.0}})

# Every detection carries its ground truth's own mask (IoU 1 >= min(thr, 1 - 1e-10) even at the threshold 1.0), two classes, two
# images, 70 pixels (a second word with 6 bits in use).  Image 0: class-2 pair on {0..9}, class-3 pair on {60..69} (across the word
# boundary).  Image 1: a class-2 pair on {5, 64}, and a padding row past num_objects = 1 that must not count.
# Every detection is a TP at every threshold: recall 1, precision 1 for both classes: AP = AP50 = AP75 = AR = 1.
CASES.append({"name": "perfect_masks", "num_classes": 4, "thresholds": [0.5, 0.75, 1.0], "max_dets": 100,
              "images": [image(70, [(0.9, 2, set(range(10))), (0.8, 3, set(range(60, 70)))], [(2, set(range(10))), (3, set(range(60, 70)))]),
                         image(70, [(0.7, 2, {5, 64})], [(2, {5, 64}), (2, {1, 2, 3})], num_objects=1)],
              "expected": {"tp": [[[1, 1], [1, 1], [1, 1]], [[1], [1], [1]]], "matched_gt": [[[0, 1], [0, 1], [0, 1]], [[0], [0], [0]]],
                           "gt_count": [0, 0, 2, 1], "AP": 1.0, "AP50": 1.0, "AP75": 1.0, "AR": 1.0}})


if __name__ == "__main__":
    doc = {"comment": "Known-answer cases for the mask metric, written by make_mask_ap_kats.py (the derivations are its comments). Masks are "
                      "0/1 rows of P pixels. 'tp' and 'matched_gt' are [image][threshold][query]; null stands for NaN.",
           "cases": CASES}
    out = Path(__file__).with_name("mask_ap_kats.json")
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print(out, out.stat().st_size, "bytes")
