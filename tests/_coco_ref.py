"""Reference for the full COCO protocol: pycocotools' COCOeval.evaluateImg and COCOeval.accumulate / summarize restated as plain
loops in NumPy fp64 - per image, per class, per area range, per threshold, with the ground truths sorted by their ignore flag and
the literal continue / break / continue scan.  Imports nothing from boosted_detr_amd and nothing from tests/_ap_ref.py (what it has
in common with that file is copied); the tests compare the kernels (include/bdetr.h K16, K17) and the host accumulate against it.

Conventions: class ids 0 (<PAD>) and 1 (<OOV>) are never a detection's label and never a ground truth; ground-truth rows
m >= num_objects do not exist; boxes are normalised COCO [x, y, w, h]; areas are in pixels of the original H x W image.
"""
import numpy as np

RECALL_THRESHOLDS = np.linspace(0.0, 1.0, 101)
COCO_AREA_RANGES = [[0.0, 1e10], [0.0, 32.0 ** 2], [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10]]
COCO_AREA_NAMES = ["all", "small", "medium", "large"]


def postprocess(cat_pred):
    """label = first maximum over classes 2 .. C-1, score = that probability (fp32, copied)."""
    cat_pred = np.asarray(cat_pred, np.float32)
    B, N, C = cat_pred.shape
    score, label = np.zeros((B, N), np.float32), np.zeros((B, N), np.int32)
    for b in range(B):
        for n in range(N):
            best = 2
            for c in range(3, C):
                if cat_pred[b, n, c] > cat_pred[b, n, best]:
                    best = c
            score[b, n], label[b, n] = cat_pred[b, n, best], best
    return score, label


# ---------------------------------------------------------------------------------------------------------------------
# IoU and area sources
# ---------------------------------------------------------------------------------------------------------------------
def box_iou(det, gt, crowd=False):
    """fp64 IoU of two fp32 COCO boxes, every operation rounded on its own; against a crowd region: inter / area(det)."""
    dx, dy, dw, dh = (np.float64(v) for v in det)
    gx, gy, gw, gh = (np.float64(v) for v in gt)
    dw, dh, gw, gh = max(dw, np.float64(0)), max(dh, np.float64(0)), max(gw, np.float64(0)), max(gh, np.float64(0))
    dx1, dy1, gx1, gy1 = dx + dw, dy + dh, gx + gw, gy + gh
    iw = max(min(dx1, gx1) - max(dx, gx), np.float64(0))
    ih = max(min(dy1, gy1) - max(dy, gy), np.float64(0))
    inter = iw * ih
    union = dw * dh if crowd else (dw * dh + gw * gh) - inter
    return inter / union if union > 0 else np.float64(0)


def box_area(box, height, width):
    """Pixels: (w * h) * (H * W) in fp64 on the clamped extents."""
    w, h = max(np.float64(box[2]), np.float64(0)), max(np.float64(box[3]), np.float64(0))
    return (w * h) * (np.float64(height) * np.float64(width))


def mask_iou(d, g, crowd=False):
    """fp64 IoU of two boolean masks: pixel counts, one division; against a crowd region: inter / count(det)."""
    d, g = np.asarray(d, bool), np.asarray(g, bool)
    inter = np.count_nonzero(d & g)
    union = np.count_nonzero(d) if crowd else np.count_nonzero(d | g)
    return np.float64(inter) / np.float64(union) if union > 0 else np.float64(0)


def mask_area(m, height, width):
    """Pixels: count * (H * W) / P in fp64, the mask's share of the original image."""
    m = np.asarray(m, bool)
    return np.float64(np.count_nonzero(m)) * (np.float64(height) * np.float64(width)) / np.float64(m.size)


def binarize(x, thr):
    """x [..., P] -> bool [..., P]: x > thr, element by element (NaN compares false)."""
    with np.errstate(invalid="ignore"):
        return np.greater(np.asarray(x, np.float32), np.float32(thr))


# ---------------------------------------------------------------------------------------------------------------------
# COCOeval.evaluateImg
# ---------------------------------------------------------------------------------------------------------------------
def match_image(score, label, det, gt_label, gt, gt_crowd, gt_area, num_objects, height, width, thresholds, area_ranges, max_dets,
                num_classes, iou_fn=box_iou, area_fn=box_area):
    """One image.  det [N,...] / gt [M,...]: boxes (iou_fn=box_iou, area_fn=box_area) or boolean masks (mask_iou, mask_area);
    gt_crowd [M] or None (no crowd); gt_area [M] in pixels or None (computed by area_fn); max_dets: the LARGEST max_det (the
    per-class truncation of evaluateImg).
    Returns dict(order [N], class_rank [N], keep [N] bool, tp / ig [A,T,N] bool, matched_gt [A,T,N] int32, gt_count [A,C],
    counters): tp = matched to a non-ignored ground truth, ig = COCOeval's dtIg."""
    score, label = np.asarray(score, np.float32), np.asarray(label, np.int64)
    N, M, T, A = len(score), len(gt_label), len(thresholds), len(area_ranges)
    order = sorted(range(N), key=lambda n: (-np.float64(score[n]), n))          # descending score, ties by ascending query index
    keep = np.zeros(N, bool)
    class_rank = np.zeros(N, np.int32)
    tp = np.zeros((A, T, N), bool)
    ig = np.zeros((A, T, N), bool)
    matched = -np.ones((A, T, N), np.int32)
    gt_count = np.zeros((A, num_classes), np.int64)
    counters = {k: np.zeros(A, np.int64) for k in ("crowd_rematch", "preferred_over_better_ignored", "unmatched_out_of_range", "tp_out_of_range")}
    real = [m for m in range(max(0, min(int(num_objects), M))) if 2 <= int(gt_label[m]) < num_classes]
    crowd = {m: bool(gt_crowd[m]) if gt_crowd is not None else False for m in real}
    area = {m: np.float64(np.float32(gt_area[m])) if gt_area is not None else area_fn(gt[m], height, width) for m in real}
    det_area = [area_fn(det[n], height, width) for n in range(N)]
    for c in sorted(set(int(l) for l in label) | set(int(gt_label[m]) for m in real)):
        every = [n for n in order if label[n] == c]
        for k, n in enumerate(every):
            class_rank[n] = k
        dets = every[:max_dets]
        for n in dets:
            keep[n] = True
        gts = [m for m in real if int(gt_label[m]) == c]
        for a, (lo, hi) in enumerate(area_ranges):
            lo, hi = np.float64(lo), np.float64(hi)
            ignore = [1 if (crowd[m] or area[m] < lo or area[m] > hi) else 0 for m in gts]
            gt_count[a, c] += sum(1 for g in ignore if g == 0)
            gtind = sorted(range(len(gts)), key=lambda i: ignore[i])            # stable: non-ignored first, each group in row order
            g_rows = [gts[i] for i in gtind]
            gt_ig = [ignore[i] for i in gtind]
            is_crowd = [crowd[m] for m in g_rows]
            ious = [[iou_fn(det[n], gt[m], crowd[m]) for m in g_rows] for n in dets]
            for t, thr in enumerate(thresholds):
                gtm = [0] * len(g_rows)                                         # 0 = free, else 1 + the detection that took it
                for di, n in enumerate(dets):
                    iou = min(np.float64(thr), 1 - 1e-10)
                    m = -1
                    for gind in range(len(g_rows)):
                        if gtm[gind] > 0 and not is_crowd[gind]:                # already matched, and not a crowd: unavailable
                            continue
                        if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:       # a regular match in hand, the ignored ones begin: stop
                            break
                        if ious[di][gind] < iou:
                            continue
                        iou, m = ious[di][gind], gind
                    if m == -1:
                        continue
                    if gt_ig[m] == 0 and any(gt_ig[j] == 1 and (gtm[j] == 0 or is_crowd[j]) and ious[di][j] > iou for j in range(len(g_rows))):
                        counters["preferred_over_better_ignored"][a] += 1
                    if gtm[m] > 0:
                        counters["crowd_rematch"][a] += 1
                    ig[a, t, n] = bool(gt_ig[m])
                    matched[a, t, n] = g_rows[m]
                    gtm[m] = 1 + n
            for n in dets:
                out = bool(det_area[n] < lo or det_area[n] > hi)
                for t in range(T):
                    if matched[a, t, n] == -1 and out:                          # dtIg |= unmatched & out of range
                        ig[a, t, n] = True
                        counters["unmatched_out_of_range"][a] += 1
                    tp[a, t, n] = matched[a, t, n] != -1 and not ig[a, t, n]
                    if tp[a, t, n] and out:
                        counters["tp_out_of_range"][a] += 1
    return {"order": np.asarray(order, np.int32), "class_rank": class_rank, "keep": keep, "tp": tp, "ig": ig, "matched_gt": matched,
            "gt_count": gt_count, "counters": counters}


def pack_bits(keep, flags, with_keep=True):
    """The kernels' uint16 words for one range: bit t = flags[t, n]; bit 15 = keep (tp_bits only)."""
    bits = np.zeros(len(keep), np.uint16)
    for n in range(len(keep)):
        w = 0x8000 if (with_keep and keep[n]) else 0
        for t in range(flags.shape[0]):
            if flags[t, n]:
                w |= 1 << t
        bits[n] = w
    return bits


# ---------------------------------------------------------------------------------------------------------------------
# COCOeval.accumulate / summarize
# ---------------------------------------------------------------------------------------------------------------------
def accumulate(images, gt_count, thresholds, max_dets):
    """images: per image, in arrival order, dict(score [N], label [N], order [N], class_rank [N], keep [N], tp [A,T,N], ig [A,T,N]).
    gt_count [A,C]: the non-ignored ground truths (npig).  Returns precision [T,R,C,A,Mx] and recall [T,C,A,Mx], -1 where npig = 0."""
    thresholds = [float(t) for t in thresholds]
    gt_count = np.asarray(gt_count)
    A, C = gt_count.shape
    T, R, Mx = len(thresholds), len(RECALL_THRESHOLDS), len(max_dets)
    precision = -np.ones((T, R, C, A, Mx))
    recall = -np.ones((T, C, A, Mx))
    for c in range(C):
        for a in range(A):
            for mi, max_det in enumerate(max_dets):
                npig = int(gt_count[a, c])
                if npig == 0:
                    continue
                scores, tps, igs = [], [], []
                for im in images:
                    for n in im["order"]:
                        if n >= 0 and im["keep"][n] and int(im["label"][n]) == c and int(im["class_rank"][n]) < max_det:
                            scores.append(np.float64(im["score"][n]))
                            tps.append([bool(im["tp"][a, t, n]) for t in range(T)])
                            igs.append([bool(im["ig"][a, t, n]) for t in range(T)])
                inds = np.argsort(-np.asarray(scores, np.float64), kind="mergesort") if scores else []
                nd = len(scores)
                for t in range(T):
                    tp_run = fp_run = 0.0
                    rc, pr = [], []
                    for i in inds:
                        if tps[i][t]:
                            tp_run += 1
                        elif not igs[i][t]:
                            fp_run += 1
                        rc.append(tp_run / npig)
                        pr.append(tp_run / (fp_run + tp_run + np.spacing(1)))
                    recall[t, c, a, mi] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = np.zeros(R)
                    at = np.searchsorted(rc, RECALL_THRESHOLDS, side="left") if nd else np.full(R, 0)
                    for ri, pi in enumerate(at):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[t, :, c, a, mi] = q
    return precision, recall


def mean_valid(a):
    a = a[a > -1]
    return float(np.mean(a)) if a.size else float("nan")


def summarize(precision, recall, thresholds, max_dets, area_names=COCO_AREA_NAMES):
    """pycocotools' summarize, for any number of ranges and max_dets: AP, AP50, AP75 (range 0, largest max_det), AP per further range,
    AR per max_det (range 0), AR per further range (largest max_det).  NaN (pycocotools: -1) where nothing is averaged."""
    thresholds = [float(t) for t in thresholds]
    last = len(max_dets) - 1

    def at_threshold(v):
        for t, thr in enumerate(thresholds):
            if abs(thr - v) < 1e-9:
                return mean_valid(precision[t, :, :, 0, last])
        return float("nan")

    out = {"AP": mean_valid(precision[:, :, :, 0, last]), "AP50": at_threshold(0.5), "AP75": at_threshold(0.75)}
    for a in range(1, len(area_names)):
        out[f"AP_{area_names[a]}"] = mean_valid(precision[:, :, :, a, last])
    for mi, m in enumerate(max_dets):
        out[f"AR_{m}"] = mean_valid(recall[:, :, 0, mi])
    for a in range(1, len(area_names)):
        out[f"AR_{area_names[a]}"] = mean_valid(recall[:, :, a, last])
    out["stats"] = [out[k] for k in list(out)]
    out["AR"] = out[f"AR_{max_dets[last]}"]
    out["per_class_AP"] = np.asarray([mean_valid(precision[:, :, c, 0, last]) for c in range(precision.shape[2])])
    return out


def evaluate(batches, thresholds, area_ranges=COCO_AREA_RANGES, max_dets=(1, 10, 100), num_classes=None, masks=False, area_names=COCO_AREA_NAMES):
    """batches: dicts of score [B,N], label [B,N], det ([B,N,4] boxes or bool [B,N,P] masks), gt_label [B,M], gt ([B,M,4] or bool
    [B,M,P]), num_objects [B], height [B], width [B], and optionally gt_crowd [B,M], gt_area [B,M] (host arrays).
    Returns (summary dict, per-image match results, (precision, recall))."""
    images, gt_count = [], np.zeros((len(area_ranges), num_classes), np.int64)
    iou_fn, area_fn = (mask_iou, mask_area) if masks else (box_iou, box_area)
    for bt in batches:
        for b in range(len(bt["score"])):
            crowd = bt["gt_crowd"][b] if bt.get("gt_crowd") is not None else None
            area = bt["gt_area"][b] if bt.get("gt_area") is not None else None
            r = match_image(bt["score"][b], bt["label"][b], bt["det"][b], bt["gt_label"][b], bt["gt"][b], crowd, area, bt["num_objects"][b],
                            bt["height"][b], bt["width"][b], thresholds, area_ranges, max(max_dets), num_classes, iou_fn, area_fn)
            r.update(score=np.asarray(bt["score"][b], np.float32), label=np.asarray(bt["label"][b]))
            gt_count += r["gt_count"]
            images.append(r)
    precision, recall = accumulate(images, gt_count, thresholds, list(max_dets))
    out = summarize(precision, recall, thresholds, list(max_dets), area_names)
    out["gt_count"] = gt_count
    return out, images, (precision, recall)
