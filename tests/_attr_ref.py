"""Reference for attribute-aware AP (include/bdetr.h K29-K31): the attribute packing, the F1 of two attribute sets, the gated matching
and the summary, as plain loops in NumPy fp64.  Imports nothing from boosted_detr_amd.  There is no second matcher: a detection (or
ground truth) travels as (geometry, attribute words, attribute count), and tests/_coco_ref.py's match_image runs once per F1 threshold
with an iou_fn that answers -1 - below every threshold - when the F1 gate fails and the plain IoU otherwise.
"""
import numpy as np

import _coco_ref as R

THR10 = np.linspace(0.5, 0.95, 10)


def attr_pack(x):
    """x [..., A] -> (bits uint64 [..., ceil(A/64)], count int32 [...]): bit a mod 64 of word a div 64 is a >= 2 and x[a] >= 0.5 in
    fp32 (NaN: not set; 0 = <PAD> and 1 = <OOV> are never an attribute)."""
    x = np.asarray(x, np.float32)
    A = x.shape[-1]
    Wa = (A + 63) // 64
    rows = x.reshape(-1, A)
    bits = [[0] * Wa for _ in range(len(rows))]
    count = np.zeros(len(rows), np.int32)
    half = np.float32(0.5)
    for r in range(len(rows)):
        for a in range(2, A):
            v = rows[r, a]
            if not np.isnan(v) and v >= half:
                bits[r][a // 64] |= 1 << (a % 64)
                count[r] += 1
    return np.asarray(bits, np.uint64).reshape(x.shape[:-1] + (Wa,)), count.reshape(x.shape[:-1])


def popcount(words):
    return sum(bin(int(w)).count("1") for w in words)


def f1(d_words, d_count, g_words, g_count, empty_f1):
    """2 tp / (count_d + count_g), one fp64 division of exact integers; empty_f1 when both sets are empty."""
    both = int(d_count) + int(g_count)
    if both == 0:
        return np.float64(empty_f1)
    tp = popcount(int(a) & int(b) for a, b in zip(d_words, g_words))
    return np.float64(2 * tp) / np.float64(both)


def passes(d, g, f1_threshold, empty_f1):
    """The gate: d, g = (geometry, words, count)."""
    return f1(d[1], d[2], g[1], g[2], empty_f1) >= min(np.float64(f1_threshold), 1 - 1e-10)


def rows_of(geometry, words, count):
    return [(geometry[i], words[i], int(count[i])) for i in range(len(geometry))]


def match_image(score, label, det, det_attr, gt_label, gt, gt_attr, gt_crowd, gt_area, num_objects, height, width, thresholds, f1_thresholds,
                empty_f1, area_ranges, max_dets, num_classes, masks=False):
    """One image.  det / gt: boxes [N,4] / [M,4] (or boolean masks with masks=True); det_attr [N,A] probabilities, gt_attr [M,A]
    multi-hot.  Returns (per F1 threshold, R.match_image's dict; the counters `redirected` and `empty_pairs`)."""
    base_iou, base_area = (R.mask_iou, R.mask_area) if masks else (R.box_iou, R.box_area)
    d_rows = rows_of(det, *attr_pack(det_attr))
    g_rows = rows_of(gt, *attr_pack(gt_attr))

    def area_fn(row, h, w):
        return base_area(row[0], h, w)

    def run(iou_fn):
        return R.match_image(score, label, d_rows, gt_label, g_rows, gt_crowd, gt_area, num_objects, height, width, thresholds, area_ranges,
                             max_dets, num_classes, iou_fn, area_fn)

    off = run(lambda d, g, crowd=False: base_iou(d[0], g[0], crowd))
    per_f = []
    for thr in f1_thresholds:
        per_f.append(run(lambda d, g, crowd=False, thr=thr: base_iou(d[0], g[0], crowd) if passes(d, g, thr, empty_f1) else np.float64(-1)))
    redirected = 0
    for n in range(len(score)):
        if any((r["matched_gt"][:, :, n] != off["matched_gt"][:, :, n]).any() for r in per_f):
            redirected += 1
    lowest = min(np.float64(t) for t in thresholds)
    empty_pairs = 0
    for n in range(len(score)):
        for m in range(max(0, min(int(num_objects), len(gt_label)))):
            if off["keep"][n] and int(gt_label[m]) == int(label[n]) and 2 <= int(gt_label[m]) < num_classes and d_rows[n][2] == 0 \
                    and g_rows[m][2] == 0 and base_iou(det[n], gt[m], False) >= lowest:
                empty_pairs += 1
    return per_f, {"redirected": redirected, "empty_pairs": empty_pairs, "gate_off": off}


def summarize(precisions, recalls, thresholds, f1_thresholds, max_dets, area_names=R.COCO_AREA_NAMES):
    """precisions[f] [T,R,C,A,Mx] and recalls[f] [T,C,A,Mx] from R.accumulate, one per F1 threshold -> the result keys.  Every mean is
    COCO's mean over the entries > -1 with f pooled into it."""
    P, Rc = np.stack(precisions), np.stack(recalls)                # [F,T,R,C,A,Mx], [F,T,C,A,Mx]
    thresholds, f1_thresholds = [float(t) for t in thresholds], [float(t) for t in f1_thresholds]
    last = len(max_dets) - 1

    def index(values, v):
        for i, x in enumerate(values):
            if abs(x - v) < 1e-9:
                return i
        return None

    def at_iou(v):
        t = index(thresholds, v)
        return float("nan") if t is None else R.mean_valid(P[:, t, :, :, 0, last])

    def at_f1(v):
        f = index(f1_thresholds, v)
        return float("nan") if f is None else R.mean_valid(P[f, :, :, :, 0, last])

    out = {"AP": R.mean_valid(P[:, :, :, :, 0, last]), "AP_IoU50": at_iou(0.5), "AP_IoU75": at_iou(0.75), "AP_F1_50": at_f1(0.5),
           "AP_F1_75": at_f1(0.75)}
    for a in range(1, len(area_names)):
        out[f"AP_{area_names[a]}"] = R.mean_valid(P[:, :, :, :, a, last])
    for mi, m in enumerate(max_dets):
        out[f"AR_{m}"] = R.mean_valid(Rc[:, :, :, 0, mi])
    for a in range(1, len(area_names)):
        out[f"AR_{area_names[a]}"] = R.mean_valid(Rc[:, :, :, a, last])
    out["stats"] = [out[k] for k in list(out)]
    out["AR"] = out[f"AR_{max_dets[last]}"]
    out["AP_table"] = [[R.mean_valid(P[f, t, :, :, 0, last]) for f in range(len(f1_thresholds))] for t in range(len(thresholds))]
    out["per_class_AP"] = np.asarray([R.mean_valid(P[:, :, :, c, 0, last]) for c in range(P.shape[3])])
    return out


def evaluate(batches, thresholds, f1_thresholds, empty_f1=1.0, area_ranges=R.COCO_AREA_RANGES, max_dets=(1, 10, 100), num_classes=None,
             masks=False, area_names=R.COCO_AREA_NAMES):
    """batches: R.evaluate's dicts plus det_attr [B,N,A] and gt_attr [B,M,A].  Returns (summary, images[f][i], counters per image)."""
    F = len(f1_thresholds)
    images = [[] for _ in range(F)]
    counters = []
    gt_count = np.zeros((len(area_ranges), num_classes), np.int64)
    for bt in batches:
        for b in range(len(bt["score"])):
            crowd = bt["gt_crowd"][b] if bt.get("gt_crowd") is not None else None
            area = bt["gt_area"][b] if bt.get("gt_area") is not None else None
            per_f, k = match_image(bt["score"][b], bt["label"][b], bt["det"][b], bt["det_attr"][b], bt["gt_label"][b], bt["gt"][b], bt["gt_attr"][b],
                                   crowd, area, bt["num_objects"][b], bt["height"][b], bt["width"][b], thresholds, f1_thresholds, empty_f1,
                                   area_ranges, max(max_dets), num_classes, masks)
            for f in range(F):
                per_f[f].update(score=np.asarray(bt["score"][b], np.float32), label=np.asarray(bt["label"][b]))
                images[f].append(per_f[f])
            gt_count += per_f[0]["gt_count"]
            counters.append(k)
    acc = [R.accumulate(images[f], gt_count, thresholds, list(max_dets)) for f in range(F)]
    out = summarize([p for p, _ in acc], [r for _, r in acc], thresholds, f1_thresholds, list(max_dets), area_names)
    out["gt_count"] = gt_count
    return out, images, counters


def records_of(images, A):
    """One batch per image as the K30 / K31 kernels would leave it: (score, label, class_rank, tp_bits [F,A,1,N], ig_bits [F,A,1,N], order).
    images[f][i] as evaluate returns them."""
    F = len(images)
    recs = []
    for i, im in enumerate(images[0]):
        tp = np.stack([np.stack([R.pack_bits(images[f][i]["keep"], images[f][i]["tp"][a]) for a in range(A)]) for f in range(F)])[:, :, None]
        ig = np.stack([np.stack([R.pack_bits(images[f][i]["keep"], images[f][i]["ig"][a], with_keep=False) for a in range(A)]) for f in range(F)])[:, :, None]
        recs.append((im["score"][None].astype(np.float32), np.asarray(im["label"], np.int32)[None], im["class_rank"][None].astype(np.int32), tp, ig,
                     np.asarray(im["order"], np.int32)[None]))
    return recs


# ---------------------------------------------------------------------------------------------------------------------
# the cases the GPU tests share (inputs only; the reference's answers are computed once per process)
# ---------------------------------------------------------------------------------------------------------------------
def draw_attributes(rng, shape, A, live=8, most=4):
    """Attribute rows [..., A] with 0 .. most of the first `live` real attributes (indices 2 .. 2 + live - 1) set: small sets, so
    F1 values on a threshold and empty / empty pairs occur."""
    rows = int(np.prod(shape))
    x = np.zeros((rows, A), np.float32)
    live = min(live, A - 2)
    for r in range(rows):
        k = int(rng.integers(0, min(most, live) + 1))
        if k:
            x[r, 2 + rng.choice(live, k, replace=False)] = 1.0
    return x.reshape(tuple(shape) + (A,))


def make_box_case(seed, B, N, M, A, C, num_objects, thresholds, f1_thresholds, hw, ranges, crowd_fraction=0.0, given_area=False, pad_row=False,
                  one_class=False):
    """Ground truths at random; a detection is a jittered copy of a ground truth of its image with that ground truth's attribute set,
    one attribute more or less, or a fresh draw; probabilities in place of the indicator on the detection side."""
    rng = np.random.default_rng(seed)
    gt_box = np.concatenate([rng.uniform(0.0, 0.6, (B, M, 2)), rng.uniform(0.05, 0.4, (B, M, 2))], -1).astype(np.float32)
    gt_label = (np.full((B, M), 2) if one_class else rng.integers(2, C, (B, M))).astype(np.int32)
    if pad_row:
        gt_label[0, 1] = 0                                        # a <PAD>-labelled row below num_objects: never a ground truth
    src = rng.integers(0, M, (B, N))
    box = (np.take_along_axis(gt_box, src[..., None], 1) + rng.normal(0, 0.02, (B, N, 4))).astype(np.float32)
    label = np.take_along_axis(gt_label, src, 1)
    label = np.where((rng.random((B, N)) < 0.15) | (label < 2), rng.integers(2, C, (B, N)), label).astype(np.int32)
    if one_class:
        label[:] = 2
    gt_attr = draw_attributes(rng, (B, M), A)
    gt_attr[..., 0] = rng.random((B, M)) < 0.5                    # what the tokenizer leaves: <PAD> / <OOV> bits set on some rows
    gt_attr[..., 1] = rng.random((B, M)) < 0.2
    own = np.take_along_axis(gt_attr, src[..., None], 1).copy()
    fresh = draw_attributes(rng, (B, N), A)
    flip = np.zeros_like(own)
    which = rng.integers(2, min(10, A), (B, N))
    np.put_along_axis(flip, which[..., None], 1.0, 2)
    kind = rng.integers(0, 4, (B, N, 1))
    hot = np.where(kind == 0, own, np.where(kind == 1, np.abs(own - flip), np.where(kind == 2, np.maximum(own, flip), fresh)))
    det_attr = np.where(hot > 0, rng.uniform(0.5, 1.0, hot.shape), rng.uniform(0.0, 0.499, hot.shape)).astype(np.float32)
    det_attr[..., :2] = rng.random((B, N, 2))                     # <PAD> / <OOV> probabilities, whatever they are
    score = rng.choice([0.125, 0.25, 0.5, 0.75, 0.9], (B, N)).astype(np.float32)
    crowd = (rng.random((B, M)) < crowd_fraction).astype(np.uint8)
    area = (rng.choice([500.0, 5000.0, 20000.0], (B, M)).astype(np.float32)) if given_area else None
    return {"score": score, "label": label, "box": box, "det_attr": det_attr, "gt_label": gt_label, "gt_box": gt_box, "gt_attr": gt_attr.astype(np.float32),
            "gt_crowd": crowd, "gt_area": area, "num_objects": np.asarray(num_objects, np.int32), "C": C, "A": A,
            "image_hw": np.tile(np.asarray(hw, np.int32).reshape(1, 2), (B, 1)), "thresholds": np.asarray(thresholds, np.float64),
            "f1_thresholds": np.asarray(f1_thresholds, np.float64), "area_ranges": np.asarray(ranges, np.float64), "max_dets": 100}


def make_mask_case(seed, B, N, M, A, C, num_objects, thresholds, f1_thresholds, hw, ranges, grid=(23, 23)):
    """make_box_case's attributes and labels on tests/_coco_cases.py's rectangle masks."""
    import _coco_cases as CS
    c = make_box_case(seed, B, N, M, A, C, num_objects, thresholds, f1_thresholds, hw, ranges, crowd_fraction=0.2)
    rng = np.random.default_rng(seed + 1000)
    h, w = grid
    gt_mask = np.stack([CS.rect_masks(rng, M, h, w) for _ in range(B)])
    src = rng.integers(0, M, (B, N))
    own = np.take_along_axis(gt_mask, src[..., None], 1)
    extra = np.stack([CS.rect_masks(rng, N, h, w, k=1) for _ in range(B)])
    kind = rng.integers(0, 3, (B, N, 1))
    mask = np.where(kind == 0, own, np.where(kind == 1, own | extra, own & ~extra))
    c.update(mask=mask, gt_mask=gt_mask, label=np.take_along_axis(c["gt_label"], src, 1).astype(np.int32))
    c["label"] = np.where(c["label"] < 2, 2, c["label"]).astype(np.int32)
    own_attr = np.take_along_axis(c["gt_attr"], src[..., None], 1)
    keep = rng.random((B, N, 1)) < 0.5                            # half of the detections carry their source's attribute set
    c["det_attr"] = np.where(keep, own_attr, c["det_attr"]).astype(np.float32)
    return c


BOX_SHAPES = {
    # B N M A T F: neither N nor M a multiple of 4, two words, crowd rows, given areas, num_objects below M, a <PAD>-labelled row
    "B2_N10_M7_A66": dict(seed=7, B=2, N=10, M=7, A=66, C=4, num_objects=[7, 5], thresholds=THR10, f1_thresholds=THR10, hw=(480, 640),
                          ranges=R.COCO_AREA_RANGES, crowd_fraction=0.25, given_area=True, pad_row=True),
    # more than 64 rows of one class: a lane owns two ground truths (`taken`'s second bit)
    "B1_N70_M70_A296": dict(seed=1, B=1, N=70, M=70, A=296, C=3, num_objects=[70], thresholds=[0.5, 0.75, 0.9], f1_thresholds=[0.5, 0.75],
                            hw=(480, 640), ranges=R.COCO_AREA_RANGES[:1], one_class=True),
}
MASK_SHAPE = dict(seed=2, B=2, N=10, M=7, A=66, C=4, num_objects=[7, 6], thresholds=THR10, f1_thresholds=[0.5, 0.75, 1.0], hw=(240, 320),
                  ranges=R.COCO_AREA_RANGES)
_CASES, _REF = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = make_mask_case(**MASK_SHAPE) if name == "mask" else make_box_case(**BOX_SHAPES[name])
    return _CASES[name]


def reference(name, f1_thresholds=None, empty_f1=1.0):
    """(per image: (per_f match results, counters)) of a shared case, computed once per (case, thresholds, empty_f1)."""
    c = case(name)
    f1s = c["f1_thresholds"] if f1_thresholds is None else np.asarray(f1_thresholds, np.float64)
    key = (name, tuple(f1s.tolist()), float(empty_f1))
    if key not in _REF:
        masks = name == "mask"
        out = []
        for b in range(len(c["score"])):
            out.append(match_image(c["score"][b], c["label"][b], c["mask" if masks else "box"][b], c["det_attr"][b], c["gt_label"][b],
                                   c["gt_mask" if masks else "gt_box"][b], c["gt_attr"][b], c["gt_crowd"][b],
                                   None if c["gt_area"] is None else c["gt_area"][b], c["num_objects"][b], c["image_hw"][b, 0], c["image_hw"][b, 1],
                                   c["thresholds"], f1s, empty_f1, c["area_ranges"], c["max_dets"], c["C"], masks))
        _REF[key] = out
    return _REF[key]
