"""The cases of the full-COCO-protocol tests (tests/test_coco_eval_cpu.py, tests/test_coco_eval_gpu.py) and the reference's answers
for them, computed once per process and shared.  make_case and rect_masks are re-created from tests/test_detection_eval_gpu.py and
tests/test_mask_eval_gpu.py (same draws in the same order, so the same inputs), not imported."""
import numpy as np

import _coco_ref as R

THR10 = np.linspace(0.5, 0.95, 10)
COCO_RANGES = np.asarray(R.COCO_AREA_RANGES, np.float64)
ALL_ONLY = COCO_RANGES[:1]


def make_case(seed, B, N, M, C, num_objects, max_dets=100, score_levels=None, crowded_class=None):
    """tests/test_detection_eval_gpu.py's generator: ground truths at random; most detections are jittered copies of a ground truth
    of their image (IoUs spread over the thresholds), labelled like it or at random."""
    rng = np.random.default_rng(seed)
    gt_box = np.concatenate([rng.uniform(0.0, 0.6, (B, M, 2)), rng.uniform(0.05, 0.4, (B, M, 2))], -1).astype(np.float32)
    gt_label = rng.integers(2, C, (B, M)).astype(np.int32)
    if crowded_class is not None:
        gt_label[:, : M // 2] = crowded_class
    src = rng.integers(0, M, (B, N))
    box = np.take_along_axis(gt_box, src[..., None], 1) + rng.normal(0, 0.03, (B, N, 4)).astype(np.float32)
    label = np.take_along_axis(gt_label, src, 1)
    swap = rng.random((B, N)) < 0.25
    label = np.where(swap, rng.integers(2, C, (B, N)), label).astype(np.int32)
    if crowded_class is not None:
        label[:, : (2 * N) // 3] = crowded_class
    score = (rng.random((B, N), dtype=np.float32) if score_levels is None else rng.choice(score_levels, (B, N))).astype(np.float32)
    return {"score": score, "label": label, "box": box.astype(np.float32), "gt_label": gt_label, "gt_box": gt_box,
            "num_objects": np.asarray(num_objects, np.int32), "C": C, "thresholds": THR10, "max_dets": max_dets}


def coco_fields(c, hw, crowd=None, gt_area=None, ranges=COCO_RANGES, max_dets=100):
    """A make_case dict completed to a K16 case: image_hw [B,2], gt_crowd uint8 [B,M] (None: none), gt_area f32 [B,M] or None."""
    B, M = c["gt_label"].shape
    c = dict(c)
    c["image_hw"] = np.tile(np.asarray(hw, np.int32).reshape(-1, 2), (B if np.ndim(hw) == 1 else 1, 1))
    c["gt_crowd"] = np.zeros((B, M), np.uint8) if crowd is None else np.asarray(crowd, np.uint8)
    c["gt_area"] = None if gt_area is None else np.asarray(gt_area, np.float32)
    c["area_ranges"], c["max_dets"] = np.asarray(ranges, np.float64), max_dets
    return c


def make_crowd_case(seed, B, N, M, C, num_objects, hw, crowd_fraction=0.2):
    """make_case's recipe with ground-truth extents uniform in [0.02, 0.4]; a fifth of the ground truths are crowd regions with
    extents x 1.5, and a detection jittered from a crowd region has extents x 0.4 (it lies inside the region: a high crowd IoU)."""
    rng = np.random.default_rng(seed)
    gt_box = np.concatenate([rng.uniform(0.0, 0.6, (B, M, 2)), rng.uniform(0.02, 0.4, (B, M, 2))], -1).astype(np.float32)
    gt_label = rng.integers(2, C, (B, M)).astype(np.int32)
    crowd = rng.random((B, M)) < crowd_fraction
    gt_box[..., 2:] *= np.where(crowd, np.float32(1.5), np.float32(1.0))[..., None]
    src = rng.integers(0, M, (B, N))
    base = np.take_along_axis(gt_box, src[..., None], 1)
    base[..., 2:] *= np.where(np.take_along_axis(crowd, src, 1), np.float32(0.4), np.float32(1.0))[..., None]
    box = base + rng.normal(0, 0.03, (B, N, 4)).astype(np.float32)
    label = np.take_along_axis(gt_label, src, 1)
    swap = rng.random((B, N)) < 0.25
    label = np.where(swap, rng.integers(2, C, (B, N)), label).astype(np.int32)
    score = rng.random((B, N), dtype=np.float32)
    c = {"score": score, "label": label, "box": box.astype(np.float32), "gt_label": gt_label, "gt_box": gt_box,
         "num_objects": np.asarray(num_objects, np.int32), "C": C, "thresholds": THR10}
    return coco_fields(c, hw, crowd)


def box_cases():
    cases = {}
    cases["crowd_N100_M130"] = make_crowd_case(11, 1, 100, 130, 6, [130], (480, 640))
    cases["B3_N50_M20"] = coco_fields(make_case(1, 3, 50, 20, 8, [0, 20, 7]), (256, 256))
    rng = np.random.default_rng(100)
    cases["off_wave_N37_M5"] = coco_fields(make_case(2, 2, 37, 5, 6, [5, 3]), [[100, 150], [333, 500]], crowd=rng.random((2, 5)) < 0.4)
    cases["duplicated_scores"] = coco_fields(make_case(4, 2, 50, 20, 5, [20, 11], score_levels=[0.125, 0.25, 0.5, 0.7]), (300, 400),
                                             crowd=rng.random((2, 20)) < 0.25)

    c = make_case(5, 2, 37, 12, 5, [12, 12])                     # duplicated ground truths: rows 2k and 2k+1 are the same object ...
    c["gt_box"][:, 1::2], c["gt_label"][:, 1::2] = c["gt_box"][:, 0::2], c["gt_label"][:, 0::2]
    c["box"][:, :6], c["label"][:, :6] = c["gt_box"][:, 0:12:2], c["gt_label"][:, 0:12:2]      # six detections sit exactly on a pair
    c["score"][:, :6] = 0.99
    crowd = np.zeros((2, 12), np.uint8)
    crowd[0, 0::2], crowd[1, 1::2] = 1, 1                        # ... and one of each pair is a crowd region: the other one is taken
    cases["duplicated_gt_one_of_each_pair_crowd"] = coco_fields(c, (480, 640), crowd)

    c = make_case(7, 2, 37, 10, 5, [4, 0])                       # rows past num_objects: the -10 padding with iscrowd = 1 garbage
    c["gt_box"][0, 4:], c["gt_box"][1, :] = -10.0, -10.0
    c["gt_box"][0, 9], c["gt_label"][0, 9] = c["box"][0, 0], c["label"][0, 0]      # matches detection 0 perfectly, but does not exist
    crowd = np.zeros((2, 10), np.uint8)
    crowd[0, 4:], crowd[1, :] = 1, 255
    cases["padding_rows_flagged_crowd"] = coco_fields(c, (480, 640), crowd, gt_area=np.full((2, 10), 5000.0))

    c = make_case(8, 2, 50, 20, 5, [20, 20])                     # every ground truth of class 3 is a crowd region: npig = 0 for it
    cases["one_class_all_crowd"] = coco_fields(c, (480, 640), c["gt_label"] == 3)

    c = make_case(9, 2, 37, 10, 5, [10, 10])                     # the annotation's area contradicts the box: the given area wins
    area = np.where(np.arange(10)[None, :] % 2 == 0, 500.0, 20000.0) * np.ones((2, 1))
    cases["gt_area_contradicts_box"] = coco_fields(c, (480, 640), rng.random((2, 10)) < 0.2, gt_area=area)
    cases["gt_area_null"] = coco_fields(c, (480, 640), cases["gt_area_contradicts_box"]["gt_crowd"])
    return cases


def rect_masks(rng, n, h, w, k=3):
    """n masks, each the union of up to k random rectangles on an h x w grid -> bool [n, h*w].  Coarse: IoU ties are dense."""
    out = np.zeros((n, h, w), bool)
    for i in range(n):
        for _ in range(rng.integers(1, k + 1)):
            y0, x0 = rng.integers(0, h), rng.integers(0, w)
            out[i, y0:y0 + rng.integers(1, max(2, h // 2)), x0:x0 + rng.integers(1, max(2, w // 2))] = True
    return out.reshape(n, h * w)


def make_mask_case(seed, B, N, M, grid, C, num_objects, hw, crowd_fraction=0.25, gt_area=None, thresholds=THR10):
    """tests/test_mask_eval_gpu.py's recipe (ground-truth masks at random; half of the detections carry a ground truth's own mask or
    that with a rectangle more or less; scores from four levels) plus crowd flags."""
    rng = np.random.default_rng(seed)
    h, w = grid
    gt_mask = np.stack([rect_masks(rng, M, h, w) for _ in range(B)])
    gt_label = rng.integers(2, C, (B, M)).astype(np.int32)
    src = rng.integers(0, M, (B, N))
    own = np.take_along_axis(gt_mask, src[..., None], 1)
    extra = np.stack([rect_masks(rng, N, h, w, k=1) for _ in range(B)])
    kind = rng.integers(0, 4, (B, N, 1))
    mask = np.where(kind == 0, own, np.where(kind == 1, own | extra, np.where(kind == 2, own & ~extra, np.stack([rect_masks(rng, N, h, w) for _ in range(B)]))))
    label = np.take_along_axis(gt_label, src, 1)
    label = np.where(rng.random((B, N)) < 0.2, rng.integers(2, C, (B, N)), label).astype(np.int32)
    score = rng.choice([0.125, 0.25, 0.5, 0.75], (B, N)).astype(np.float32)
    crowd = rng.random((B, M)) < crowd_fraction
    c = {"score": score, "label": label, "mask": mask, "gt_label": gt_label, "gt_mask": gt_mask, "num_objects": np.asarray(num_objects, np.int32),
         "C": C, "thresholds": np.asarray(thresholds, np.float64)}
    return coco_fields(c, hw, crowd, gt_area)


def mask_cases():
    cases = {}
    cases["P529_B2_N60_M70"] = make_mask_case(21, 2, 60, 70, (23, 23), 6, [70, 33], (240, 320))          # M > 64: a lane owns two rows
    cases["P70_B2_N37_M12"] = make_mask_case(22, 2, 37, 12, (5, 14), 5, [12, 9], [[120, 160], [200, 200]])  # the tail word in play
    area = np.where(np.arange(12)[None, :] % 3 == 0, 100.0, 8000.0) * np.ones((2, 1))
    cases["P70_gt_area_given"] = make_mask_case(22, 2, 37, 12, (5, 14), 5, [12, 9], [[120, 160], [200, 200]], gt_area=area)
    return cases


BOX_CASES = box_cases()
MASK_CASES = mask_cases()
_REF = {}


def reference(name):
    """(per-image match results) of the reference for a box or mask case, computed once and shared."""
    if name not in _REF:
        masks = name in MASK_CASES
        c = (MASK_CASES if masks else BOX_CASES)[name]
        B = len(c["score"])
        images = []
        for b in range(B):
            images.append(R.match_image(c["score"][b], c["label"][b], c["mask" if masks else "box"][b], c["gt_label"][b],
                                        c["gt_mask" if masks else "gt_box"][b], c["gt_crowd"][b], None if c["gt_area"] is None else c["gt_area"][b],
                                        c["num_objects"][b], c["image_hw"][b, 0], c["image_hw"][b, 1], c["thresholds"], c["area_ranges"],
                                        c["max_dets"], c["C"], R.mask_iou if masks else R.box_iou, R.mask_area if masks else R.box_area))
        _REF[name] = images
    return _REF[name]
