"""GPU half of the image-resolution mask path (csrc/maskimage.hip): bdetr_mask_upsample_bits (K19), bdetr_mask_source_bits (K20) and
bdetr_mask_inter (K21) bit for bit against the NumPy references (tests/_mask_image_ref.py, tests/_mask_raster_ref.py),
bdetr_mask_match_coco_inter (K22) against bdetr_mask_match_coco (K17) and against tests/_coco_ref.py, and
Model.evaluate(coco=True, mask_resolution="image") end to end."""
import functools
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import _coco_cases as CS
import _coco_ref as R
import _mask_image_ref as MI
import _mask_raster_ref as RR

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = 23
# a one-word row, an exact word, a partial last word, three words, h < G and h > G: one launch
SIZES = [(1, 1), (5, 7), (23, 23), (64, 64), (65, 63), (37, 130)]
ONES = -1                                            # int64 with every bit set: what the output buffers are pre-filled with


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def host_bits(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# K19
# ---------------------------------------------------------------------------------------------------------------------
def test_upsample_bits_bit_for_bit(cuda):
    from boosted_detr_amd import kernels as K
    rng = np.random.default_rng(19)
    B, N = len(SIZES), 3
    L = (3.0 * rng.standard_normal((B, N, G, G))).astype(np.float32)
    L[:, 0][rng.random((B, G, G)) < 0.1] = 0.0       # exact zeros: v = 0 sets no bit
    L[:, 2] = -np.abs(L[:, 2]) - 0.5                 # an all-negative map: an empty mask
    L[2, 1, 4, 5], L[3, 1, 7, 7], L[4, 1, 0, 0], L[5, 1, 22, 22] = np.inf, -np.inf, np.nan, np.inf
    L[5, 0, 10, 3], L[5, 0, 11, 9] = np.nan, -np.inf
    hw = np.asarray(SIZES, np.int32)
    Hm, Wm = MI.layout(hw)
    assert (Hm, Wm) == (65, 3) == K.mask_layout(hw)
    out = torch.full((B, N, Hm, Wm), ONES, dtype=torch.int64, device=DEV)
    bits, pop = K.mask_upsample_bits(dev(L), dev(hw), Hm, Wm, out=out)
    assert bits is out and pop.dtype == torch.int32 and tuple(pop.shape) == (B, N)
    got, got_pop = host_bits(bits), pop.cpu().numpy()
    nonempty = 0
    for b, (h, w) in enumerate(SIZES):
        for n in range(N):
            mask = MI.upsample_mask(L[b, n], h, w)
            want = MI.pack(mask, Hm, Wm)             # zero at x >= w and y >= h: the pre-filled ones must be gone
            assert np.array_equal(got[b, n], want), (b, n, (h, w), np.argwhere(got[b, n] != want)[:4].tolist())
            assert got_pop[b, n] == int(mask.sum()), (b, n)
            nonempty += int(mask.any())
        assert got_pop[b, 2] == 0
    assert nonempty >= B
    again, again_pop = K.mask_upsample_bits(dev(L), dev(hw), Hm, Wm)
    assert torch.equal(again, bits) and torch.equal(again_pop, pop)
    # a wider layout than the images need (another batch's Hm, Wm) only adds zeros
    wide, wide_pop = K.mask_upsample_bits(dev(L), dev(hw), 70, 4, out=torch.full((B, N, 70, 4), ONES, dtype=torch.int64, device=DEV))
    wide = host_bits(wide)
    assert np.array_equal(wide[:, :, :Hm, :Wm], got) and not wide[:, :, Hm:].any() and not wide[..., Wm:].any() and torch.equal(wide_pop, pop)


# ---------------------------------------------------------------------------------------------------------------------
# K20
# ---------------------------------------------------------------------------------------------------------------------
def _kats():
    return json.loads((Path(__file__).parent / "golden" / "mask_raster_kats.json").read_text())["cases"]


@functools.lru_cache(maxsize=None)
def source_cases():
    """(records, want): one record per size with every polygon and RLE shape of tests/test_mask_targets_gpu.py and an object without
    a segmentation, one record per hand-derived known answer (the polygon, and the same mask as RLE); want[b][m] = bool [h, w]."""
    from test_mask_targets_gpu import polygon_cases, rle_cases
    records, want = [], []
    for (h, w) in SIZES:
        segs = list(polygon_cases(h, w).values()) + [{"size": [h, w], "counts": c} for c in rle_cases(h, w).values()]
        segs.insert(3, None)
        records.append({"height": h, "width": w, "segmentation": segs})
        want.append([RR.segmentation_mask(s, h, w) for s in segs])
    for c in _kats():
        known = np.asarray([[ch == "1" for ch in row] for row in c["mask"]])
        records.append({"height": c["h"], "width": c["w"],
                        "segmentation": [c["rings"], {"size": [c["h"], c["w"]], "counts": RR.mask_to_counts(known)}]})
        want.append([known, known])
    for r in records:
        n = len(r["segmentation"])
        r.update(bbox=[[0.0, 0.0, 1.0, 1.0]] * n, category=[["x"]] * n)
    return records, want


def test_source_bits_bit_for_bit(cuda):
    from boosted_detr_amd import kernels as K
    from boosted_detr_amd import pipeline
    records, want = source_cases()
    pack = pipeline.pad_annotations(records, with_masks=True)["segments"]
    B, M = pack["kind"].shape
    hw = np.asarray([[r["height"], r["width"]] for r in records], np.int32)
    Hm, Wm = MI.layout(hw)
    assert (Hm, Wm) == (65, 3) and M >= 19 and (pack["kind"] == 0).any() and (pack["kind"] == 1).any() and (pack["kind"] == 2).any()
    out = torch.full((B, M, Hm, Wm), ONES, dtype=torch.int64, device=DEV)
    bits, pop = K.mask_source_bits(pack["items"], pack["item_off"], pack["kind"], pack["hw"], Hm, Wm, out=out)
    got, got_pop = host_bits(bits), pop.cpu().numpy()
    for b, r in enumerate(records):
        for m in range(M):
            mask = want[b][m] if m < len(want[b]) else np.zeros((r["height"], r["width"]), bool)      # padding rows: kind 0
            packed = MI.pack(mask, Hm, Wm)
            assert np.array_equal(got[b, m], packed), (b, m, np.argwhere(got[b, m] != packed)[:4].tolist())
            assert got_pop[b, m] == int(mask.sum()), (b, m)
    # pop is bdetr_mask_targets' area on the same pack
    place = np.tile(np.asarray([[1, 1, 1, 1, 0, 0]], np.int32), (B, 1))
    _, area = K.mask_targets(pack["items"], pack["item_off"], pack["kind"], pack["hw"], place, 23)
    assert torch.equal(area, pop) and int(pop.sum()) > 0
    again, again_pop = K.mask_source_bits(pack["items"], pack["item_off"], pack["kind"], pack["hw"], Hm, Wm)
    assert torch.equal(again, bits) and torch.equal(again_pop, pop)


def test_source_bits_over_several_bands(cuda):
    """3100 rows of one word: more rows than one LDS band holds (3072 words), so the polygon and the RLE both cross a band border."""
    from boosted_detr_amd import kernels as K
    from boosted_detr_amd import pipeline
    h, w = 3100, 40
    rings = [[3.2, 10.5, 36.7, 2900.25, 20.0, 3099.5, 1.5, 1500.0], [10.0, 3060.0, 30.0, 3060.0, 30.0, 3090.0, 10.0, 3090.0]]
    counts = [3000, 150, 2 * h - 3150 + 3065, 20, 38 * h - 3085]          # a run from column 0 into column 1, one across row 3072
    assert sum(counts) == h * w
    segs = [rings, {"size": [h, w], "counts": counts}]
    rec = {"height": h, "width": w, "segmentation": segs, "bbox": [[0.0, 0.0, 1.0, 1.0]] * 2, "category": [["x"]] * 2}
    pack = pipeline.pad_annotations([rec], with_masks=True)["segments"]
    bits, pop = K.mask_source_bits(pack["items"], pack["item_off"], pack["kind"], pack["hw"], h, 1,
                                   out=torch.full((1, 2, h, 1), ONES, dtype=torch.int64, device=DEV))
    got, got_pop = host_bits(bits), pop.cpu().numpy()
    for m, s in enumerate(segs):
        mask = RR.segmentation_mask(s, h, w)
        assert mask[3071:3073].any() and np.array_equal(got[0, m], MI.pack(mask, h, 1)) and got_pop[0, m] == int(mask.sum()), m


# ---------------------------------------------------------------------------------------------------------------------
# K21
# ---------------------------------------------------------------------------------------------------------------------
def _random_bits(rng, *shape):
    dense = rng.integers(0, 1 << 63, shape, dtype=np.int64) | (rng.integers(0, 2, shape, dtype=np.int64) << 63)
    return np.where(rng.random(shape) < 0.3, dense & rng.integers(0, 1 << 62, shape, dtype=np.int64), dense)


@pytest.mark.parametrize("name,B,N,M,Hm,Wm,num_objects", [
    ("past_one_wave_both_ways", 3, 70, 70, 64, 1, [0, 1, 70]),           # 64 words: 16-byte loads
    ("odd_word_count", 2, 5, 3, 37, 3, [3, 2]),                          # (37, 130): 111 words, 8-byte loads
    ("two_word_splits", 1, 9, 9, 300, 8, [9]),                           # 2400 words: two workgroups share every mask pair
])
def test_inter_equals_numpy(cuda, name, B, N, M, Hm, Wm, num_objects):
    from boosted_detr_amd import kernels as K
    rng = np.random.default_rng(len(name))
    d, g = _random_bits(rng, B, N, Hm, Wm), _random_bits(rng, B, M, Hm, Wm)
    nobj = dev(np.asarray(num_objects, np.int32))
    got = K.mask_inter(dev(d), dev(g), nobj)
    want = MI.inter(d, g, num_objects)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), name
    assert want.any() and all((want[b, :, n:] == 0).all() for b, n in enumerate(num_objects))
    assert torch.equal(K.mask_inter(dev(d), dev(g), nobj), got)          # integer adds: two calls are bit-identical


# ---------------------------------------------------------------------------------------------------------------------
# K22
# ---------------------------------------------------------------------------------------------------------------------
def _grid_operands(c):
    from boosted_detr_amd import kernels as K
    from test_coco_eval_gpu import as_logits
    det_bits, det_pop = K.mask_binarize(dev(as_logits(c["mask"])), 0.0)
    gt_bits, gt_pop = K.mask_binarize(dev(c["gt_mask"].astype(np.float32)), 0.5)
    return det_bits, det_pop, gt_bits, gt_pop


def _run_inter_match(c, inter, det_pop, gt_pop, pix):
    from boosted_detr_amd import kernels as K
    from test_coco_eval_gpu import to_host
    gt_count = torch.zeros(len(c["area_ranges"]), c["C"], dtype=torch.int32, device=DEV)
    out = K.mask_match_coco_inter(dev(c["score"]), dev(c["label"]), inter, det_pop, dev(c["gt_label"]), gt_pop, dev(c["gt_crowd"]),
                                  None if c["gt_area"] is None else dev(c["gt_area"]), dev(c["num_objects"]), dev(c["image_hw"]), pix,
                                  dev(c["area_ranges"]), c["thresholds"], c["C"], c["max_dets"], gt_count)
    return to_host(*out) + (gt_count,)


K17_CASES = dict(CS.MASK_CASES)
# 130 x 130 x 4 bytes of intersections do not fit the 64 KiB of LDS: the kernel reads them from memory
K17_CASES["inter_not_staged_N130_M130"] = CS.make_mask_case(23, 1, 130, 130, (5, 14), 5, [130], (120, 160))


@pytest.mark.parametrize("name", list(K17_CASES))
def test_match_from_inter_equals_k17(cuda, name):
    from test_coco_eval_gpu import run_mask
    c = K17_CASES[name]
    B, N, P = c["mask"].shape
    det_bits, det_pop, gt_bits, gt_pop = _grid_operands(c)
    inter = MI.inter(host_bits(det_bits)[:, :, None, :], host_bits(gt_bits)[:, :, None, :], c["gt_label"].shape[0] * [c["gt_label"].shape[1]])
    got = _run_inter_match(c, dev(inter), det_pop, gt_pop, torch.full((B,), P, dtype=torch.int32, device=DEV))
    want = run_mask(c)
    for k, what in enumerate(("order", "class_rank", "tp_bits", "ig_bits", "matched_gt")):
        assert np.array_equal(got[k], want[k]), (name, what)
    assert torch.equal(got[5], want[5]) and (got[2] & 0x3FF).any() and got[3].any()
    assert (4 * N * c["gt_label"].shape[1] > 60 * 1024) == name.startswith("inter_not_staged")


@functools.lru_cache(maxsize=None)
def image_case(with_area):
    """Two images of different sizes; masks are unions of rectangles at image resolution, half of the detections a ground truth's own
    mask or that with a rectangle more or less; crowd rows; optionally the annotations' areas.  -> (case, reference images)."""
    rng = np.random.default_rng(31)
    sizes, N, M, C = [(37, 130), (64, 64)], 40, 9, 5
    num_objects = [9, 6]
    det, gt, srcs = [], [], []
    for (h, w) in sizes:
        g = CS.rect_masks(rng, M, h, w)
        src = rng.integers(0, M, N)
        srcs.append(src)
        own, extra = g[src], CS.rect_masks(rng, N, h, w, k=1)
        kind = rng.integers(0, 4, (N, 1))
        det.append(np.where(kind == 0, own, np.where(kind == 1, own | extra, np.where(kind == 2, own & ~extra, CS.rect_masks(rng, N, h, w)))))
        gt.append(g)
    gt_label = rng.integers(2, C, (2, M)).astype(np.int32)
    label = np.where(rng.random((2, N)) < 0.2, rng.integers(2, C, (2, N)), np.take_along_axis(gt_label, np.stack(srcs), 1)).astype(np.int32)
    score = rng.choice([0.125, 0.25, 0.5, 0.75], (2, N)).astype(np.float32)
    crowd = (rng.random((2, M)) < 0.3).astype(np.uint8)
    area = np.where(np.arange(M)[None, :] % 3 == 0, 100.0, 3000.0) * np.ones((2, 1)) if with_area else None
    c = {"score": score, "label": label, "det": det, "gt": gt, "gt_label": gt_label, "gt_crowd": crowd,
         "gt_area": None if area is None else area.astype(np.float32), "num_objects": np.asarray(num_objects, np.int32), "C": C,
         "thresholds": CS.THR10, "area_ranges": CS.COCO_RANGES, "max_dets": 100, "image_hw": np.asarray(sizes, np.int32)}
    images = [R.match_image(score[b], label[b], det[b], gt_label[b], gt[b], crowd[b], None if area is None else c["gt_area"][b], num_objects[b],
                            h, w, CS.THR10, CS.COCO_RANGES, 100, C, R.mask_iou, R.mask_area) for b, (h, w) in enumerate(sizes)]
    return c, images


@pytest.mark.parametrize("with_area", [False, True])
def test_match_at_image_size_against_reference(cuda, with_area):
    from boosted_detr_amd import kernels as K
    from test_coco_eval_gpu import assert_bit_exact
    c, images = image_case(with_area)
    sizes = [tuple(v) for v in c["image_hw"].tolist()]
    Hm, Wm = MI.layout(c["image_hw"])
    d = np.stack([np.stack([MI.pack(m.reshape(h, w), Hm, Wm) for m in c["det"][b]]) for b, (h, w) in enumerate(sizes)])
    g = np.stack([np.stack([MI.pack(m.reshape(h, w), Hm, Wm) for m in c["gt"][b]]) for b, (h, w) in enumerate(sizes)])
    det_pop = np.stack([m.sum(axis=1) for m in c["det"]]).astype(np.int32)
    gt_pop = np.stack([m.sum(axis=1) for m in c["gt"]]).astype(np.int32)
    inter = K.mask_inter(dev(d.view(np.int64)), dev(g.view(np.int64)), dev(c["num_objects"]))
    pix = dev(np.asarray([h * w for h, w in sizes], np.int32))
    got = _run_inter_match(c, inter, dev(det_pop), dev(gt_pop), pix)
    assert_bit_exact(f"image_sizes_area_{with_area}", images, got)
    counters = {k: sum(im["counters"][k] for im in images) for k in images[0]["counters"]}
    assert counters["crowd_rematch"][0] > 0 and (got[2] & 0x3FF).any() and got[3].any() and (got[5].cpu().numpy().sum(1) > 0)[:2].all()
    if with_area:
        assert not np.array_equal(got[5].cpu().numpy(), sum(im["gt_count"] for im in image_case(False)[1]))


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator: a batch over the byte budget is refused and the next one is scored
# ---------------------------------------------------------------------------------------------------------------------
def _evaluator_batch(rng, sizes, N, C):
    from boosted_detr_amd import pipeline
    records = []
    for (h, w) in sizes:
        segs = [[[0.2 * w, 0.2 * h, 0.8 * w, 0.2 * h, 0.8 * w, 0.7 * h, 0.2 * w, 0.7 * h]], {"size": [h, w], "counts": [h, h * (w - 1)]}]
        records.append({"height": h, "width": w, "bbox": [[0.2, 0.2, 0.6, 0.5], [0.0, 0.0, 0.1, 1.0]], "category": [["a"], ["b"]],
                        "iscrowd": [0, 1], "area": [float(h * w) / 4, float(h)], "segmentation": segs})
    pad = pipeline.pad_annotations(records, with_eval_fields=True, with_masks=True)
    B = len(sizes)
    cat_pred = rng.random((B, N, C), dtype=np.float32)
    logits = (3.0 * rng.standard_normal((B, N, G, G))).astype(np.float32)
    cat_ids = rng.integers(2, C, (B, 2)).astype(np.int32)
    return pad, dev(cat_pred), dev(logits), dev(cat_ids), dev(np.full(B, 2, np.int32))


def test_batch_over_the_budget_is_refused_and_the_next_one_is_scored(cuda):
    from boosted_detr_amd.evaluation import CocoImageMaskEvaluator, host_image_hw
    rng = np.random.default_rng(4)
    N, C = 7, 5
    big = _evaluator_batch(rng, [(200, 300), (100, 100)], N, C)
    small = _evaluator_batch(rng, [(20, 30), (12, 70)], N, C)
    need_small = 8 * 20 * 2 * 2 * (N + 2)
    ev, fresh = CocoImageMaskEvaluator(C, max_mask_bytes=need_small), CocoImageMaskEvaluator(C)
    for e, batches in ((ev, (big, small)), (fresh, (small,))):
        for pad, cat_pred, logits, cat_ids, num_objects in batches:
            hw = host_image_hw(pad["height"], pad["width"])
            if pad is big[0] and e is ev:
                with pytest.raises(ValueError, match="max_mask_bytes"):
                    e.update(cat_pred, logits, cat_ids, pad["segments"], num_objects, hw, pad["iscrowd"], pad["area"])
                assert e._kept == [] and e._gt_count is None          # nothing was launched, nothing was kept
            else:
                e.update(cat_pred, logits, cat_ids, pad["segments"], num_objects, hw, pad["iscrowd"], pad["area"])
    a, b = ev.result(), fresh.result()
    assert a["num_images"] == b["num_images"] == 2 and a["num_detections"] == 2 * N
    assert all(a["stats"][k] == b["stats"][k] or (math.isnan(a["stats"][k]) and math.isnan(b["stats"][k])) for k in range(12))
    assert np.array_equal(a["gt_count_per_range"], b["gt_count_per_range"]) and a["num_ground_truths"] == 2          # the crowd rows are not counted


# ---------------------------------------------------------------------------------------------------------------------
# end to end: the small head model of tests/test_panoptic_train_gpu.py (64 x 64 inputs, 30 queries); the images' ORIGINAL sizes differ
# ---------------------------------------------------------------------------------------------------------------------
ORIGINAL = [[(48, 80), (100, 60)], [(64, 64), (33, 130)]]          # per batch, per image: (height, width)


def _image_records(i):
    """Two images with 2 and 4 objects (as _small_head_batch's num_objects): polygons, RLE, an object without a segmentation, a
    crowd region, and one 2 x 2 pixel object that a single cell of the 23 x 23 grid swallows."""
    (h0, w0), (h1, w1) = ORIGINAL[i]
    rng = np.random.default_rng(50 + i)
    first = {"height": h0, "width": w0, "iscrowd": [0, 1],
             "segmentation": [[[0.1 * w0, 0.2 * h0, 0.7 * w0, 0.15 * h0, 0.6 * w0, 0.8 * h0]],
                              {"size": [h0, w0], "counts": [h0 * 3 + 5, h0 * (w0 // 2), h0 * w0 - h0 * 3 - 5 - h0 * (w0 // 2)]}]}
    second = {"height": h1, "width": w1, "iscrowd": [0, 0, 1 if i else 0, 0],
              "segmentation": [[[0.05 * w1, 0.05 * h1, 0.5 * w1, 0.05 * h1, 0.5 * w1, 0.6 * h1, 0.05 * w1, 0.6 * h1],
                                [0.4 * w1, 0.5 * h1, 0.95 * w1, 0.5 * h1, 0.95 * w1, 0.95 * h1]],
                               [[10.0, 10.0, 12.0, 10.0, 12.0, 12.0, 10.0, 12.0]],
                               {"size": [h1, w1], "counts": [h1 // 2, h1 * 4, h1 * w1 - h1 // 2 - h1 * 4]}, None]}
    for r in (first, second):
        n = len(r["segmentation"])
        r.update(bbox=[[0.1, 0.1, 0.5, 0.5]] * n, category=[["x"]] * n, area=rng.choice([400.0, 3000.0, 50000.0], n).tolist())
    return [first, second]


def _attach(batch, records):
    """The image-resolution keys of pad_annotations next to the pre-tokenised ones, and the grid targets of the same segmentations."""
    from boosted_detr_amd import pipeline
    pad = pipeline.pad_annotations(records, max_objects=5, with_eval_fields=True, with_masks=True)
    batch.update({k: pad[k] for k in ("segments", "iscrowd", "area", "height", "width")})
    batch["masks"] = pipeline.mask_targets(pad)["masks"]
    return batch


@pytest.fixture(scope="module")
def trained(cuda):
    from boosted_detr_amd import kernels as K
    from boosted_detr_amd.training import SGD
    from test_panoptic_train_gpu import _small_head_batch, _small_head_model
    prev = K.set_deterministic(True)                 # the reference below repeats evaluate's forward passes: they must give the same bits
    try:
        records = [_image_records(0), _image_records(1)]
        batches = [_attach(_small_head_batch(9), records[0]), _attach(_small_head_batch(21), records[1])]
        model = _small_head_model()
        model.compile(optimizer=SGD(learning_rate=1e-3, momentum=.9, nesterov=True, clipnorm=.1))
        for i in range(3):
            model.train_step(batches[i % 2])
        # a briefly trained model finds nothing: make the two objects of the second batch's first image the model's own
        # image-resolution segmentations (as RLE), one of them a crowd region
        h, w = ORIGINAL[1][0]
        seg = model.segmentations(batches[1], resolution="image")
        on = seg["image_mask_area"][0].cpu().numpy()
        pick = [n for n in range(on.size) if 0 < on[n] < h * w][:2]
        assert len(pick) == 2, on.tolist()
        own = [MI.unpack(host_bits(seg["image_masks"][0, n]), h, w) for n in pick]
        records[1][0]["segmentation"] = [{"size": [h, w], "counts": RR.mask_to_counts(m)} for m in own]
        _attach(batches[1], records[1])
        batches[1]["category"][0, :2] = seg["labels"][0, pick]
        batches[1]["bbox"][0, :2] = seg["boxes"][0, pick]
        torch.cuda.synchronize()
        yield batches, records, model
    finally:
        K.set_deterministic(prev)


def test_evaluate_at_image_resolution_end_to_end(trained):
    from boosted_detr_amd.evaluation import CocoImageMaskEvaluator
    from test_coco_eval_gpu import STAT_KEYS, exactly, state_of
    batches, records, model = trained
    C, both = model.num_categories, ("bbox", "segm")
    model.predict_raw(batches[0])                    # the user's last call
    users_masks = model.panoptic_masks().clone()
    before = state_of(model)
    grid = model.evaluate(batches, coco=True, iou_types=both)
    mask_ev = CocoImageMaskEvaluator(C)
    res = model.evaluate(batches, coco=True, iou_types=both, mask_resolution="image", mask_evaluator=mask_ev)
    by_class = model.evaluate(batches, iou_types="segm", mask_evaluator=CocoImageMaskEvaluator(C))      # the evaluator's class selects the path
    torch.cuda.synchronize()
    after = state_of(model)
    assert before[1] == after[1] and set(before[0]) == set(after[0]) and len(before[0]) > 100
    for k, t in before[0].items():
        assert torch.equal(t, after[0][k]), k        # weights, moving statistics, optimizer slots: bit-identical
    assert torch.equal(model.panoptic_masks(), users_masks)
    assert set(res) == set(grid) and len(res["mask_stats"]) == 12
    for k in STAT_KEYS + ("AR",):
        assert exactly(res[k], grid[k]), k           # the box numbers do not know the keyword
        assert exactly(by_class["mask_" + k], res["mask_" + k]), k
    assert np.array_equal(res["per_class_AP"], grid["per_class_AP"], equal_nan=True)

    # the reference: segmentations()' logits through the NumPy rule, the segmentations through the plain-loop rasteriser
    ref_batches = []
    for i, b in enumerate(batches):
        seg = model.segmentations(b, resolution="image")
        cat, _, _ = model.predict_raw(b)
        logits = seg["mask_logits"].cpu().numpy()
        assert logits.shape == (2, 30, G, G) and seg["image_hw"].cpu().tolist() == [list(v) for v in ORIGINAL[i]]
        Hm, Wm = MI.layout(ORIGINAL[i])
        got_bits, got_pop = host_bits(seg["image_masks"]), seg["image_mask_area"].cpu().numpy()
        det, gt = [], []
        for k, (h, w) in enumerate(ORIGINAL[i]):
            masks = [MI.upsample_mask(logits[k, n], h, w) for n in range(30)]
            assert all(np.array_equal(got_bits[k, n], MI.pack(m, Hm, Wm)) and got_pop[k, n] == m.sum() for n, m in enumerate(masks)), (i, k)
            det.append(np.stack([m.reshape(-1) for m in masks]))
            segs = records[i][k]["segmentation"] + [None] * (5 - len(records[i][k]["segmentation"]))
            gt.append(np.stack([RR.segmentation_mask(s, h, w).reshape(-1) for s in segs]))
        score, label = R.postprocess(cat.cpu().numpy())
        ref_batches.append({"score": score, "label": label, "det": det, "gt": gt, "gt_label": b["category"].cpu().numpy(),
                            "num_objects": b["num_objects"].cpu().numpy(), "gt_crowd": b["iscrowd"], "gt_area": b["area"],
                            "height": b["height"], "width": b["width"]})
    model.predict_raw(batches[0])
    ref, images, _ = R.evaluate(ref_batches, CS.THR10, num_classes=C, masks=True)
    rec, gt_count = mask_ev._to_host()               # what the kernels left: integers, compared bit for bit
    for i, im in enumerate(images):
        score, label, class_rank, tp_bits, ig_bits, order = (r[:, i % 2] if r.ndim == 3 else r[i % 2] for r in rec[i // 2])
        assert np.array_equal(order, im["order"]) and np.array_equal(class_rank, im["class_rank"]), i
        for a in range(4):
            assert np.array_equal(tp_bits[a], R.pack_bits(im["keep"], im["tp"][a])), (i, a)
            assert np.array_equal(ig_bits[a], R.pack_bits(im["keep"], im["ig"][a], with_keep=False)), (i, a)
    assert np.array_equal(gt_count, ref["gt_count"])
    for i, k in enumerate(STAT_KEYS):
        assert exactly(res["mask_" + k], ref[k]), (k, res["mask_" + k], ref[k])
        assert exactly(res["mask_stats"][i], ref["stats"][i])
    assert exactly(res["mask_AR"], ref["AR_100"]) and np.array_equal(res["per_class_mask_AP"], ref["per_class_AP"], equal_nan=True)
    assert res["mask_AP"] > 0.0 and res["num_images"] == 4 and sum(im["ig"].any() for im in images) > 0
    # the grid blurs what the image resolution keeps: the numbers differ on this data
    assert any(not exactly(res["mask_" + k], grid["mask_" + k]) for k in STAT_KEYS), [(res["mask_" + k], grid["mask_" + k]) for k in STAT_KEYS]

    it = model.optimizer.iterations                  # and training goes on as if nothing had happened
    logs = model.logs_to_host(model.train_step(batches[0]))
    assert math.isfinite(logs["loss"]) and model.optimizer.iterations == it + 1


def test_detection_ap_passes_the_resolution_through(trained):
    from boosted_detr_amd.training import DetectionAP
    batches, _, model = trained
    cb = DetectionAP(batches, iou_types=("bbox", "segm"), coco=True, mask_resolution="image")
    cb.set_model(model)
    logs = {}
    cb.on_epoch_end(0, logs)
    want = model.evaluate(batches, coco=True, iou_types=("bbox", "segm"), mask_resolution="image")
    assert logs["val_mask_AP"] == want["mask_AP"] and logs["val_AP"] == want["AP"] and "val_mask_AR_small" in logs
