"""Plain-loop NumPy reference of the panoptic path (include/bdetr.h, K23-K26) and of the PQ accumulate.  Imports nothing from the
product; builds on tests/_mask_image_ref.py (upsample, pack, unpack).

Everything is integers or K19's fp64 rule, so the GPU tests compare bit for bit; PQ / SQ / RQ are Python floats summed in
(batch, image, row) order."""
import numpy as np

import _mask_image_ref as MI


# ---------------------------------------------------------------------------------------------------------------------
# K23
# ---------------------------------------------------------------------------------------------------------------------
def select(score, label, is_stuff, threshold):
    """score float32 [N], label [N], is_stuff [C] or None -> seg_of int [N]."""
    score, thr = np.asarray(score, np.float32), np.float32(threshold)
    N = score.shape[0]
    seg_of = [-1] * N
    for n in range(N):
        if not (score[n] > thr):                     # NaN: dropped
            continue
        seg_of[n] = n
        l = int(label[n])
        if is_stuff is not None and 0 <= l < len(is_stuff) and is_stuff[l]:
            for j in range(n):
                if seg_of[j] >= 0 and int(label[j]) == l:
                    seg_of[n] = j
                    break
    return np.asarray(seg_of, np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# K24
# ---------------------------------------------------------------------------------------------------------------------
def merge(logits, seg_of, h, w):
    """logits float32 [N,G,G], seg_of [N] -> ids int64 [h,w]: per pixel the kept query with the largest value > 0 (a tie: the lowest
    query; NaN never wins) gives its seg_of; -1 where there is none."""
    N = logits.shape[0]
    best = np.zeros((h, w), np.float64)
    winner = np.full((h, w), -1, np.int64)
    for n in range(N):                               # ascending: `>` keeps the lower query on a tie
        if not 0 <= int(seg_of[n]) < N:
            continue
        v = MI.upsample(logits[n], h, w)
        with np.errstate(invalid="ignore"):
            better = np.greater(v, best)             # NaN > x is False
        best[better] = v[better]
        winner[better] = n
    ids = np.full((h, w), -1, np.int64)
    ids[winner >= 0] = np.asarray(seg_of, np.int64)[winner[winner >= 0]]
    return ids


def ids_canvas(ids, Hm, Wm):
    """ids [h,w] -> int16 [Hm, 64 Wm] with -1 outside the image."""
    out = np.full((Hm, 64 * Wm), -1, np.int16)
    out[:ids.shape[0], :ids.shape[1]] = ids
    return out


def bits_of_ids(ids, N, Hm, Wm):
    """ids [h,w] -> (bits uint64 [N,Hm,Wm], pop int64 [N]): row s holds the pixels with id s."""
    bits = np.stack([MI.pack(ids == s, Hm, Wm) for s in range(N)])
    pop = np.asarray([int((ids == s).sum()) for s in range(N)], np.int64)
    return bits, pop


# ---------------------------------------------------------------------------------------------------------------------
# K25
# ---------------------------------------------------------------------------------------------------------------------
def gt_exclusive(masks, gt_label, num_objects, C):
    """masks bool [M,h,w] (may overlap) -> (exclusive bool [M,h,w], gt_ids int64 [h,w] with -1 = void, gt_pop int64 [M]): rows at or
    past num_objects and labels outside [2, C) are no segments; a pixel belongs to the lowest segment row that covers it."""
    masks = np.asarray(masks, bool)
    M, h, w = masks.shape
    out = np.zeros_like(masks)
    gt_ids = np.full((h, w), -1, np.int64)
    for m in range(M):
        if m >= num_objects or not 2 <= int(gt_label[m]) < C:
            continue
        for y in range(h):
            for x in range(w):
                if masks[m, y, x] and gt_ids[y, x] < 0:
                    gt_ids[y, x] = m
                    out[m, y, x] = True
    return out, gt_ids, out.reshape(M, -1).sum(axis=1).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# K21's result, from the two id maps (no bitmask is ANDed here)
# ---------------------------------------------------------------------------------------------------------------------
def joint_counts(pred_ids, gt_ids, N, M):
    inter = np.zeros((N, M), np.int64)
    h, w = pred_ids.shape
    for y in range(h):
        for x in range(w):
            if pred_ids[y, x] >= 0 and gt_ids[y, x] >= 0:
                inter[pred_ids[y, x], gt_ids[y, x]] += 1
    return inter


# ---------------------------------------------------------------------------------------------------------------------
# K26
# ---------------------------------------------------------------------------------------------------------------------
def match(inter, pred_pop, pred_label, seg_of, gt_pop, gt_label, gt_crowd, num_objects, C, min_area):
    """-> dict(gt_state [M], pred_state [N], match_inter [M], match_union [M]); panopticapi's pq_compute_single_core in integers."""
    N, M = inter.shape
    need = max(int(min_area), 1)
    pred_seg = [int(seg_of[n]) == n and int(pred_pop[n]) >= need for n in range(N)]
    gt_seg = [m < num_objects and 2 <= int(gt_label[m]) < C and int(gt_pop[m]) >= 1 for m in range(M)]
    crowd = [bool(gt_seg[m] and gt_crowd is not None and gt_crowd[m]) for m in range(M)]
    void = [int(pred_pop[n]) - sum(int(inter[n, m]) for m in range(M)) for n in range(N)]
    gt_state = [(-2 if crowd[m] else -1) if gt_seg[m] else -3 for m in range(M)]
    pred_state = [-1 if pred_seg[n] else -3 for n in range(N)]
    match_inter, match_union = [0] * M, [0] * M
    for n in range(N):
        for m in range(M):
            if not (pred_seg[n] and gt_seg[m]) or crowd[m] or int(pred_label[n]) != int(gt_label[m]):
                continue
            i = int(inter[n, m])
            union = int(pred_pop[n]) + int(gt_pop[m]) - i - void[n]
            if 2 * i > union:
                assert pred_state[n] == -1 and gt_state[m] == -1, "two matches for one segment: the maps are not disjoint"
                pred_state[n], gt_state[m] = m, n
                match_inter[m], match_union[m] = i, union
    for n in range(N):
        if pred_state[n] != -1:
            continue
        on_crowd = sum(int(inter[n, m]) for m in range(M) if crowd[m] and int(gt_label[m]) == int(pred_label[n]))
        if 2 * (void[n] + on_crowd) > int(pred_pop[n]):
            pred_state[n] = -2
    return {"gt_state": np.asarray(gt_state, np.int64), "pred_state": np.asarray(pred_state, np.int64),
            "match_inter": np.asarray(match_inter, np.int64), "match_union": np.asarray(match_union, np.int64)}


# ---------------------------------------------------------------------------------------------------------------------
# the accumulate
# ---------------------------------------------------------------------------------------------------------------------
def pq(images, C, stuff_classes=()):
    """images: in (batch, image) order, dicts with gt_state / match_inter / match_union / gt_label [M] and pred_state / pred_label [N].
    -> dict with tp / fp / fn [C], per-class and averaged PQ / SQ / RQ (all classes, _th, _st) as Python floats."""
    tp, fp, fn, iou = [0] * C, [0] * C, [0] * C, [0.0] * C
    for im in images:
        for m in range(len(im["gt_state"])):
            c, s = int(im["gt_label"][m]), int(im["gt_state"][m])
            if s >= 0:
                tp[c] += 1
                iou[c] += float(int(im["match_inter"][m])) / float(int(im["match_union"][m]))
            elif s == -1:
                fn[c] += 1
        for n in range(len(im["pred_state"])):
            if int(im["pred_state"][n]) == -1:
                fp[int(im["pred_label"][n])] += 1
    out = {"tp": tp, "fp": fp, "fn": fn, "per_class": {}}
    for c in range(C):
        if tp[c] + fp[c] + fn[c] == 0:
            continue
        denom = tp[c] + 0.5 * fp[c] + 0.5 * fn[c]
        out["per_class"][c] = (iou[c] / denom, iou[c] / tp[c] if tp[c] else 0.0, tp[c] / denom)
    for suffix, keep in (("", lambda c: True), ("_th", lambda c: c not in stuff_classes), ("_st", lambda c: c in stuff_classes)):
        rows = [v for c, v in sorted(out["per_class"].items()) if keep(c)]
        n = len(rows)
        for k, name in enumerate(("PQ", "SQ", "RQ")):
            out[name + suffix] = sum(r[k] for r in rows) / n if n else 0.0
        out["num_classes_scored" + suffix] = n
    return out


def image_reference(logits, score, label, is_stuff, threshold, masks, gt_label, gt_crowd, num_objects, C, min_area, h, w):
    """One image through select, merge, the exclusive ground truth, the joint counts and the matching.  masks bool [M,h,w]."""
    N, M = logits.shape[0], len(gt_label)
    seg_of = select(score, label, is_stuff, threshold)
    ids = merge(logits, seg_of, h, w)
    pred_pop = np.asarray([int((ids == s).sum()) for s in range(N)], np.int64)
    excl, gt_ids, gt_pop = gt_exclusive(masks, gt_label, num_objects, C)
    inter = joint_counts(ids, gt_ids, N, M)
    out = match(inter, pred_pop, label, seg_of, gt_pop, gt_label, gt_crowd, num_objects, C, min_area)
    out.update(seg_of=seg_of, ids=ids, pred_pop=pred_pop, gt_ids=gt_ids, gt_pop=gt_pop, gt_excl=excl, inter=inter,
               gt_label=np.asarray(gt_label, np.int64), pred_label=np.asarray(label, np.int64))
    return out
