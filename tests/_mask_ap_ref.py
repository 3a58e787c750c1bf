"""Reference for the mask metric: COCOeval's evaluateImg for iouType="segm" (no crowd, all areas, one max_dets) restated as plain
NumPy loops over boolean masks, and the word packing the kernels use.  Shares no code with the product (boosted_detr_amd.evaluation
is not imported here); the accumulate, the postprocess and the tp_bits packing are tests/_ap_ref.py's, unchanged.

Conventions (include/bdetr.h, K15): a mask is a row of P pixels; a prediction's pixel is on when its logit is > 0, a target's when
its value is > 0.5 (NaN: off); class ids 0 and 1 are never a ground truth; ground-truth rows m >= num_objects do not exist.
"""
import numpy as np

from _ap_ref import accumulate, pack_bits, postprocess  # noqa: F401  (re-exported for the tests)


def binarize(x, thr):
    """x [..., P] -> bool [..., P]: x > thr, element by element (NaN compares false)."""
    with np.errstate(invalid="ignore"):
        return np.greater(np.asarray(x, np.float32), np.float32(thr))


def pack_words(mask):
    """bool [P] -> uint64 [ceil(P/64)]: pixel p is bit p mod 64 of word p div 64; unused bits are zero."""
    mask = np.asarray(mask, bool)
    words = [0] * ((mask.size + 63) // 64)
    for p in range(mask.size):
        if mask[p]:
            words[p // 64] |= 1 << (p % 64)
    return np.asarray(words, np.uint64)


def mask_iou(d, g):
    """fp64 IoU of two boolean masks: pixel counts, one division; 0 when the union is empty."""
    d, g = np.asarray(d, bool), np.asarray(g, bool)
    inter = np.count_nonzero(d & g)
    union = np.count_nonzero(d | g)
    return np.float64(inter) / np.float64(union) if union > 0 else np.float64(0)


def match_image(score, label, mask, gt_label, gt_mask, num_objects, thresholds, max_dets, num_classes):
    """One image; mask bool [N,P], gt_mask bool [M,P].  _ap_ref.match_image with mask_iou in place of the box IoU.
    Returns dict(order [N], keep [N] bool, tp [T,N] bool, matched_gt [T,N] int32, gt_count [C])."""
    score, label = np.asarray(score, np.float32), np.asarray(label, np.int64)
    N, M, T = len(score), len(gt_label), len(thresholds)
    order = sorted(range(N), key=lambda n: (-np.float64(score[n]), n))          # descending score, ties by ascending query index
    keep = np.zeros(N, bool)
    tp = np.zeros((T, N), bool)
    matched = -np.ones((T, N), np.int32)
    gt_count = np.zeros(num_classes, np.int64)
    real = [m for m in range(max(0, min(int(num_objects), M))) if 2 <= int(gt_label[m]) < num_classes]
    for m in real:
        gt_count[int(gt_label[m])] += 1
    for c in sorted(set(int(l) for l in label)):
        dets = [n for n in order if label[n] == c][:max_dets]
        for n in dets:
            keep[n] = True
        gts = [m for m in real if int(gt_label[m]) == c]
        ious = [[mask_iou(mask[n], gt_mask[m]) for m in gts] for n in dets]
        for t, thr in enumerate(thresholds):
            taken = [False] * len(gts)
            for di, n in enumerate(dets):
                best = min(np.float64(thr), 1 - 1e-10)
                found = -1
                for gi in range(len(gts)):
                    if taken[gi]:
                        continue
                    if ious[di][gi] < best:
                        continue
                    best, found = ious[di][gi], gi
                if found == -1:
                    continue
                taken[found] = True
                tp[t, n] = True
                matched[t, n] = gts[found]
    return {"order": np.asarray(order, np.int32), "keep": keep, "tp": tp, "matched_gt": matched, "gt_count": gt_count}


def evaluate(batches, thresholds, max_dets, num_classes):
    """batches: dicts of score [B,N], label [B,N], mask bool [B,N,P], gt_label [B,M], gt_mask bool [B,M,P], num_objects [B] (host
    arrays).  Returns (metrics, per-image match results)."""
    images, gt_count = [], np.zeros(num_classes, np.int64)
    for bt in batches:
        for b in range(len(bt["score"])):
            r = match_image(bt["score"][b], bt["label"][b], bt["mask"][b], bt["gt_label"][b], bt["gt_mask"][b], bt["num_objects"][b],
                            thresholds, max_dets, num_classes)
            r.update(score=np.asarray(bt["score"][b], np.float32), label=np.asarray(bt["label"][b]))
            gt_count += r["gt_count"]
            images.append(r)
    return accumulate(images, gt_count, thresholds), images
