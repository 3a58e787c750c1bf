"""GPU half of the panoptic-quality path (csrc/panopticmerge.hip): bdetr_panoptic_select (K23), bdetr_panoptic_merge (K24),
bdetr_panoptic_gt_exclusive (K25) and bdetr_panoptic_match (K26, fed by bdetr_mask_inter) against the plain-loop reference
(tests/_panoptic_ref.py) - exactly for every integer and bitmask, within 1e-12 for PQ / SQ / RQ (only the order of a sum may
differ) - and Model.evaluate_panoptic / panoptic_segmentation / training.PanopticQuality end to end."""
import math

import numpy as np
import pytest
import torch

import _coco_ref as R
import _mask_image_ref as MI
import _mask_raster_ref as RR
import _panoptic_cases as PC
import _panoptic_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
# a partial last word, a width one past a word boundary, rows past h, words wholly outside an image
SIZES = [(37, 70), (64, 129)]
HM, WM = 64, 3
N, M, C = 9, 6, 7


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def host_bits(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# K23
# ---------------------------------------------------------------------------------------------------------------------
def test_select(cuda):
    from boosted_detr_amd import kernels as K
    thr = 0.85
    at = np.float32(thr)
    # image 0: three queries of the stuff class 3 of which the first is below the threshold; a score equal to the threshold; a NaN
    score = np.asarray([[0.5, 0.9, at, 0.95, np.nan, 0.99, 0.9, np.nextafter(at, np.float32(1)), 0.1],
                        [0.9, 0.9, 0.9, 0.2, 0.99, 0.86, 0.0, 1.0, 0.9]], np.float32)
    label = np.asarray([[3, 3, 3, 2, 2, 3, 2, 4, 4], [5, 5, 2, 5, 5, 2, 2, 6, 2]], np.int32)
    stuff = np.asarray([0, 0, 0, 1, 0, 1, 0], np.uint8)
    for flags in (stuff, None):
        got = K.panoptic_select(dev(score), dev(label), thr, C, None if flags is None else dev(flags))
        want = np.stack([P.select(score[b], label[b], flags, thr) for b in range(2)])
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (flags is None, got.cpu().tolist())
    assert want[0].tolist() == [-1, 1, -1, 3, -1, 5, 6, 7, -1]
    assert K.panoptic_select(dev(score), dev(label), thr, C, dev(stuff)).cpu().numpy()[0].tolist() == [-1, 1, -1, 3, -1, 1, 6, 7, -1]
    # more queries than one pass of the workgroup, every class a stuff class, threshold 0
    rng = np.random.default_rng(23)
    score = rng.random((3, 300), dtype=np.float32)
    score[rng.random((3, 300)) < 0.3] = 0.0
    label = rng.integers(2, C, (3, 300)).astype(np.int32)
    got = K.panoptic_select(dev(score), dev(label), 0.0, C, dev(np.ones(C, np.uint8))).cpu().numpy()
    want = np.stack([P.select(score[b], label[b], np.ones(C, np.uint8), 0.0) for b in range(3)])
    assert np.array_equal(got, want) and len(set(want[0][want[0] >= 0].tolist())) == C - 2


# ---------------------------------------------------------------------------------------------------------------------
# K24
# ---------------------------------------------------------------------------------------------------------------------
def run_merge(L, seg_of, sizes, Hm, Wm):
    """bdetr_panoptic_merge against the reference, exactly: ids (with -1 outside the image), bits, pop, disjointness, two calls,
    and the call without bits.  Returns the reference's id maps."""
    from boosted_detr_amd import kernels as K
    B, n = L.shape[:2]
    hw = dev(np.asarray(sizes, np.int32))
    ids, bits, pop = K.panoptic_merge(dev(L), dev(seg_of.astype(np.int32)), hw, Hm, Wm)
    assert ids.dtype == torch.int16 and tuple(ids.shape) == (B, Hm, 64 * Wm) and bits.dtype == torch.int64 and pop.dtype == torch.int32
    got_ids, got_bits, got_pop = ids.cpu().numpy(), host_bits(bits), pop.cpu().numpy()
    maps = []
    for b, (h, w) in enumerate(sizes):
        want = P.merge(L[b], seg_of[b], h, w)
        maps.append(want)
        canvas = P.ids_canvas(want, Hm, Wm)
        assert np.array_equal(got_ids[b], canvas), (b, np.argwhere(got_ids[b] != canvas)[:4].tolist())
        want_bits, want_pop = P.bits_of_ids(want, n, Hm, Wm)
        assert np.array_equal(got_bits[b], want_bits), (b, np.argwhere(got_bits[b] != want_bits)[:4].tolist())
        assert np.array_equal(got_pop[b], want_pop), (b, got_pop[b].tolist(), want_pop.tolist())
        # pairwise disjoint: the OR over the rows is "some id", and the counts add up to its pixels
        assert np.array_equal(np.bitwise_or.reduce(got_bits[b], axis=0), MI.pack(want >= 0, Hm, Wm))
        assert int(got_pop[b].sum()) == int(MI.popcount(np.bitwise_or.reduce(got_bits[b], axis=0).reshape(1, -1))[0]) == int((want >= 0).sum())
    again = K.panoptic_merge(dev(L), dev(seg_of.astype(np.int32)), hw, Hm, Wm)
    assert torch.equal(again[0], ids) and torch.equal(again[1], bits) and torch.equal(again[2], pop)          # identical bytes
    ids2, none, pop2 = K.panoptic_merge(dev(L), dev(seg_of.astype(np.int32)), hw, Hm, Wm, with_bits=False)
    assert none is None and torch.equal(ids2, ids) and torch.equal(pop2, pop)
    return maps


@pytest.mark.parametrize("G", [5, 23])
def test_merge_base_case(cuda, G):
    rng = np.random.default_rng(24 + G)
    L = (3.0 * rng.standard_normal((2, N, G, G))).astype(np.float32)
    L[:, 0][rng.random((2, G, G)) < 0.1] = 0.0       # exact zeros: v = 0 claims nothing
    L[0, 2, 1, 1], L[1, 4, G - 1, 0], L[1, 2, 2, 3], L[0, 7, 0, 0] = np.inf, -np.inf, np.nan, np.nan
    # self, dropped, merged into an earlier query (stuff), an id outside [0, N) (not kept)
    seg_of = np.asarray([[0, -1, 2, 2, 4, -1, 0, 7, 8], [-1, 1, 1, 3, -1, 5, 6, 1, N]], np.int64)
    maps = run_merge(L, seg_of, SIZES, HM, WM)
    assert all(len(set(m[m >= 0].tolist())) >= 3 for m in maps)
    assert all(1 not in m and 5 not in m for m in maps[:1]) and N not in maps[1]
    # a wider layout than the images need only adds void
    from boosted_detr_amd import kernels as K
    ids, bits, pop = K.panoptic_merge(dev(L), dev(seg_of.astype(np.int32)), dev(np.asarray(SIZES, np.int32)), 70, 4)
    base = K.panoptic_merge(dev(L), dev(seg_of.astype(np.int32)), dev(np.asarray(SIZES, np.int32)), HM, WM)
    ids, bits = ids.cpu().numpy(), host_bits(bits)
    assert np.array_equal(ids[:, :HM, :64 * WM], base[0].cpu().numpy()) and (ids[:, HM:] == -1).all() and (ids[:, :, 64 * WM:] == -1).all()
    assert np.array_equal(bits[:, :, :HM, :WM], host_bits(base[1])) and not bits[:, :, HM:].any() and not bits[..., WM:].any()
    assert torch.equal(pop, base[2])


def test_merge_rules(cuda):
    from boosted_detr_amd import kernels as K
    G = 5
    rng = np.random.default_rng(7)
    L = (3.0 * rng.standard_normal((2, N, G, G))).astype(np.float32)
    none = np.full((2, N), -1, np.int64)
    # two kept queries with identical logits: the lower index owns every pixel
    tie = L.copy()
    tie[:, 6] = tie[:, 3]
    seg = none.copy()
    seg[:, 3], seg[:, 6] = 3, 6
    maps = run_merge(tie, seg, SIZES, HM, WM)
    assert all((m == 3).any() and not (m == 6).any() for m in maps)
    # all logits <= 0: everything is void
    maps = run_merge(-np.abs(L), np.tile(np.arange(N), (2, 1)), SIZES, HM, WM)
    assert all((m == -1).all() for m in maps)
    # a NaN logit poisons the pixels it touches for that query only; another query takes them
    nan = np.abs(L) + 0.5
    nan[:, 0] += 100.0
    nan[:, 0, 2, 2] = np.nan
    maps = run_merge(nan, np.tile(np.arange(N), (2, 1)), SIZES, HM, WM)
    assert all((m == 0).any() and (m > 0).any() and not (m < 0).any() for m in maps)
    # no query kept
    maps = run_merge(L, none, SIZES, HM, WM)
    assert all((m == -1).all() for m in maps)
    # exactly one kept query: its row is bdetr_mask_upsample_bits' row, bit for bit
    seg = none.copy()
    seg[0, 4], seg[1, 8] = 4, 8
    run_merge(L, seg, SIZES, HM, WM)
    hw = dev(np.asarray(SIZES, np.int32))
    _, bits, pop = K.panoptic_merge(dev(L), dev(seg.astype(np.int32)), hw, HM, WM)
    up_bits, up_pop = K.mask_upsample_bits(dev(L), hw, HM, WM)
    for b, n in ((0, 4), (1, 8)):
        assert torch.equal(bits[b, n], up_bits[b, n]) and int(pop[b, n]) == int(up_pop[b, n]) > 0
        assert int(pop[b].sum()) == int(pop[b, n]) and not bits[b, :n].any() and not bits[b, n + 1:].any()


@pytest.mark.parametrize("kept", ["all", "five"])
def test_merge_more_queries_than_lds_holds(cuda, kept):
    """130 kept queries at G = 23 are 275 KB of logits, more than a CU's LDS; with five of the 130 kept the compaction is what is run."""
    n, G = 130, 23
    rng = np.random.default_rng(130)
    L = (3.0 * rng.standard_normal((1, n, G, G))).astype(np.float32)
    seg_of = np.arange(n)[None].copy()
    if kept == "five":
        seg_of[:] = -1
        seg_of[0, [3, 64, 65, 100, 129]] = [3, 64, 3, 100, 129]
    maps = run_merge(L, seg_of, [(40, 70)], 40, 2)
    assert len(set(maps[0][maps[0] >= 0].tolist())) >= (60 if kept == "all" else 4)


# ---------------------------------------------------------------------------------------------------------------------
# K25
# ---------------------------------------------------------------------------------------------------------------------
def _gt_records():
    """Per image 7 rows: two overlapping polygons, a polygon with label 0 over both, a row without a segmentation, an RLE over the
    first two, a polygon wholly inside the first (hidden), and a polygon at m >= num_objects = 6."""
    records = []
    for (h, w) in SIZES:
        def box(x0, y0, x1, y1):
            return [[x0 * w, y0 * h, x1 * w, y0 * h, x1 * w, y1 * h, x0 * w, y1 * h]]
        rle = {"size": [h, w], "counts": [h * (w // 3) + 2, h * (w // 3), h * w - 2 * h * (w // 3) - 2]}
        segs = [box(0.1, 0.1, 0.6, 0.7), box(0.4, 0.3, 0.9, 0.9), box(0.0, 0.0, 1.0, 0.5), None, rle, box(0.2, 0.2, 0.4, 0.4),
                box(0.05, 0.8, 0.3, 0.95)]
        records.append({"height": h, "width": w, "segmentation": segs, "bbox": [[0.0, 0.0, 1.0, 1.0]] * 7, "category": [["x"]] * 7})
    return records


GT_LABEL = np.asarray([[2, 3, 0, 4, 5, 6, 2]] * 2, np.int32)


def test_gt_exclusive(cuda):
    from boosted_detr_amd import kernels as K
    from boosted_detr_amd import pipeline
    records = _gt_records()
    pack = pipeline.pad_annotations(records, with_masks=True)["segments"]
    assert pack["kind"].shape == (2, 7) and (pack["kind"][:, 3] == 0).all()
    bits, pop0 = K.mask_source_bits(pack["items"], pack["item_off"], pack["kind"], pack["hw"], HM, WM)
    before = host_bits(bits).copy()
    nobj = np.asarray([6, 6], np.int32)
    gt_pop = K.panoptic_gt_exclusive(bits, dev(GT_LABEL), dev(nobj), C)
    got, got_pop = host_bits(bits), gt_pop.cpu().numpy()
    for b, (h, w) in enumerate(SIZES):
        masks = np.stack([RR.segmentation_mask(s, h, w) for s in records[b]["segmentation"]])
        assert np.array_equal(before[b], np.stack([MI.pack(m, HM, WM) for m in masks]))
        excl, gt_ids, want_pop = P.gt_exclusive(masks, GT_LABEL[b], 6, C)
        assert np.array_equal(got[b], np.stack([MI.pack(m, HM, WM) for m in excl])), b
        assert np.array_equal(got_pop[b], want_pop), (got_pop[b], want_pop)
        # the label-0 row, the row without a segmentation, the hidden row and the row past num_objects are empty; the label-0
        # row hid nothing although it covers both polygons; the overlaps went to the lower row
        assert masks[2].any() and masks[5].any() and masks[6].any() and (masks[0] & masks[1]).any() and (masks[4] & masks[0]).any()
        assert want_pop[[2, 3, 5, 6]].tolist() == [0, 0, 0, 0] and want_pop[0] == masks[0].sum() and 0 < want_pop[1] < masks[1].sum()
        assert 0 < want_pop[4] < masks[4].sum()
    again = K.panoptic_gt_exclusive(bits, dev(GT_LABEL), dev(nobj), C)          # idempotent, and integer adds only
    assert torch.equal(again, gt_pop) and np.array_equal(host_bits(bits), got)


# ---------------------------------------------------------------------------------------------------------------------
# K21 + K26
# ---------------------------------------------------------------------------------------------------------------------
def device_match(pred_ids, n, pred_label, seg_of, gt_masks, gt_label, gt_crowd, num_objects, num_classes, min_area):
    """One image from its id map and ground-truth masks through K25, K21 and K26 -> (host outputs dict, reference dict)."""
    from boosted_detr_amd import kernels as K
    h, w = pred_ids.shape
    Hm, Wm = h, (w + 63) // 64
    m = len(gt_label)
    bits, pop = P.bits_of_ids(pred_ids, n, Hm, Wm)
    gt_bits = dev(np.stack([MI.pack(g, Hm, Wm) for g in gt_masks]).view(np.int64)[None])
    nobj = dev(np.asarray([num_objects], np.int32))
    gl = dev(np.asarray(gt_label, np.int32)[None])
    gt_pop = K.panoptic_gt_exclusive(gt_bits, gl, nobj, num_classes)
    inter = K.mask_inter(dev(bits.view(np.int64)[None]), gt_bits, nobj)
    crowd = None if gt_crowd is None else dev(np.asarray(gt_crowd, np.uint8)[None])
    out = K.panoptic_match(inter, dev(pop.astype(np.int32)[None]), dev(np.asarray(pred_label, np.int32)[None]),
                           dev(np.asarray(seg_of, np.int32)[None]), gt_pop, gl, crowd, nobj, num_classes, min_area)
    assert all(t.dtype == torch.int32 for t in out)
    got = {k: t.cpu().numpy()[0] for k, t in zip(("gt_state", "pred_state", "match_inter", "match_union"), out)}
    got.update(inter=inter.cpu().numpy()[0], gt_pop=gt_pop.cpu().numpy()[0], gt_label=np.asarray(gt_label), pred_label=np.asarray(pred_label))
    _, gt_ids, want_pop = P.gt_exclusive(gt_masks, gt_label, num_objects, num_classes)
    want_inter = P.joint_counts(pred_ids, gt_ids, n, m)             # from the two id maps: no bitmask is ANDed on this side
    assert np.array_equal(got["inter"], want_inter) and np.array_equal(got["gt_pop"], want_pop)
    want = P.match(want_inter, pop, pred_label, seg_of, want_pop, gt_label, gt_crowd, num_objects, num_classes, min_area)
    for k in ("gt_state", "pred_state", "match_inter", "match_union"):
        assert np.array_equal(got[k], want[k]), (k, got[k].tolist(), want[k].tolist())
    return got, want


@pytest.mark.parametrize("name", list(PC.CASES))
def test_match_hand_worked_cases(cuda, name):
    from boosted_detr_amd.evaluation import PanopticEvaluator
    c = PC.CASES[name]
    want = c["want"]
    got, _ = device_match(c["pred_ids"], PC.N, c["pred_label"], c["seg_of"], c["gt_masks"], c["gt_label"], c["gt_crowd"], c["num_objects"],
                          PC.C, c["min_area"])
    assert got["pred_state"].tolist() == want["pred_state"] and got["gt_state"].tolist() == want["gt_state"]
    for k in ("match_inter", "match_union"):
        if k in want:
            assert got[k].tolist() == want[k]
    keys = ("gt_state", "pred_state", "match_inter", "match_union", "gt_label", "pred_label")
    res = PanopticEvaluator(PC.C, min_area=c["min_area"]).result_from([tuple(got[k][None].astype(np.int32) for k in keys)])
    assert (int(res["tp"].sum()), int(res["fp"].sum()), int(res["fn"].sum())) == (want["tp"], want["fp"], want["fn"])
    assert all(abs(res[k] - want[k]) <= 1e-12 for k in ("PQ", "SQ", "RQ")) and res["num_classes_scored"] == want["classes"]


@pytest.mark.parametrize("crowd", [True, False])
def test_match_random_maps_past_one_workgroup_pass(cuda, crowd):
    """300 queries and 300 ground-truth rows on a 64 x 128 image: more rows than the workgroup has lanes, so both of its loops
    stride; segments are blocks of a grid, half of the predictions a ground truth's own block or that with a neighbour's."""
    rng = np.random.default_rng(26)
    n = m = 300
    h, w = 64, 128
    cell = (np.arange(h)[:, None] // 4) * 16 + (np.arange(w)[None, :] // 8)          # 16 x 16 blocks of 4 x 8 pixels: ids 0..255
    gt_ids = np.where(rng.random(256) < 0.85, rng.permutation(256), -1)[cell]
    shift = np.roll(cell, rng.integers(0, 5), axis=1)
    pred_ids = np.where(rng.random(256) < 0.85, np.arange(256), -1)[np.where(rng.random((h, w)) < 0.7, cell, shift)] + 30
    pred_ids[pred_ids == 29] = -1
    gt_masks = np.stack([gt_ids == k for k in range(m)])
    gt_masks[5] |= gt_masks[4]                                                       # an overlap for K25 to remove
    gt_label = rng.integers(2, 5, m).astype(np.int32)
    gt_label[7] = 1
    pred_label = rng.integers(2, 5, n).astype(np.int32)
    seg_of = np.arange(n)
    seg_of[40:50] = -1
    min_area = 20
    got, want = device_match(pred_ids, n, pred_label, seg_of, gt_masks, gt_label, (rng.random(m) < 0.2) if crowd else None, 280, 5, min_area)
    assert (want["pred_state"] >= 0).sum() >= 5 and (want["pred_state"] == -1).any() and (want["gt_state"] == -1).any()
    assert (want["pred_state"] == -3).any() and ((want["gt_state"] == -2).any() == crowd)
    assert ((want["pred_state"] == -2).any() or not crowd)


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator on the base case: every kernel chained, against the reference per image
# ---------------------------------------------------------------------------------------------------------------------
def test_evaluator_chain_on_the_base_case(cuda):
    from boosted_detr_amd import pipeline
    from boosted_detr_amd.evaluation import PanopticEvaluator
    G, thr, min_area, stuff = 5, 0.3, 40, (3,)
    rng = np.random.default_rng(99)
    records = [dict(r, segmentation=r["segmentation"][:M], bbox=r["bbox"][:M], category=r["category"][:M]) for r in _gt_records()]
    pad = pipeline.pad_annotations(records, max_objects=M, with_masks=True)
    gt_label = GT_LABEL[:, :M].copy()
    gt_label[:, 2] = 4                                # (the label-0 row of _gt_records becomes a real segment here)
    crowd = np.zeros((2, M), np.uint8)
    crowd[:, 4] = 1
    nobj = np.asarray([6, 5], np.int32)
    cat_pred = rng.random((2, N, C), dtype=np.float32)
    cat_pred /= cat_pred.sum(axis=2, keepdims=True)
    cat_pred[:, :, 2:] *= 2.5
    L = (3.0 * rng.standard_normal((2, N, G, G))).astype(np.float32)
    hw = np.asarray(SIZES, np.int32)
    score, label = R.postprocess(cat_pred)
    images = []
    for b, (h, w) in enumerate(SIZES):
        masks = np.stack([RR.segmentation_mask(s, h, w) for s in records[b]["segmentation"]])
        is_stuff = np.zeros(C, np.uint8)
        is_stuff[list(stuff)] = 1
        images.append(P.image_reference(L[b], score[b], label[b], is_stuff, thr, masks, gt_label[b], crowd[b], int(nobj[b]), C, min_area, h, w))
    want = P.pq(images, C, stuff)
    ev = PanopticEvaluator(C, score_threshold=thr, min_area=min_area, stuff_classes=stuff)
    for _ in range(2):                                # reset() starts over
        ev.reset()
        ev.update(dev(cat_pred), dev(L).reshape(2, N, G * G), dev(gt_label), pad["segments"], dev(nobj), hw, crowd)
    (rec,) = ev._to_host()
    for b, im in enumerate(images):
        for k, key in enumerate(("gt_state", "pred_state", "match_inter", "match_union", "gt_label", "pred_label")):
            assert np.array_equal(rec[k][b], im[key]), (b, key, rec[k][b].tolist(), im[key].tolist())
        assert np.array_equal(ev.last["seg_of"][b].cpu().numpy(), im["seg_of"]) and np.array_equal(ev.last["pred_pop"][b].cpu().numpy(), im["pred_pop"])
        assert np.array_equal(ev.last["gt_pop"][b].cpu().numpy(), im["gt_pop"]) and np.array_equal(ev.last["inter"][b].cpu().numpy(), im["inter"])
    got = ev.result()
    assert got["tp"].tolist() == want["tp"] and got["fp"].tolist() == want["fp"] and got["fn"].tolist() == want["fn"] and got["num_images"] == 2
    for s in ("", "_th", "_st"):
        assert all(abs(got[k + s] - want[k + s]) <= 1e-12 for k in ("PQ", "SQ", "RQ")), (s, got, want)
    assert sum(want["fp"]) > 0 and sum(want["fn"]) > 0 and any((im["seg_of"] >= 0).sum() >= 3 for im in images)


# ---------------------------------------------------------------------------------------------------------------------
# end to end: the small head model of tests/test_panoptic_train_gpu.py (64 x 64 inputs, 30 queries); the images' ORIGINAL sizes differ
# ---------------------------------------------------------------------------------------------------------------------
MIN_AREA = 30


@pytest.fixture(scope="module")
def trained(cuda):
    from boosted_detr_amd import kernels as K
    from boosted_detr_amd.training import SGD
    from test_mask_image_eval_gpu import ORIGINAL, _attach, _image_records
    from test_panoptic_train_gpu import _small_head_batch, _small_head_model
    prev = K.set_deterministic(True)                 # the reference below repeats the forward passes: they must give the same bits
    try:
        records = [_image_records(0), _image_records(1)]
        batches = [_attach(_small_head_batch(9), records[0]), _attach(_small_head_batch(21), records[1])]
        model = _small_head_model()
        model.compile(optimizer=SGD(learning_rate=1e-3, momentum=.9, nesterov=True, clipnorm=.1))
        for i in range(3):
            model.train_step(batches[i % 2])
        # a briefly trained model is sure of nothing: keep the upper half of its queries, and call its most frequent class stuff
        # ... and it finds nothing: make the two objects of the second batch's first image two of its own segments (as RLE).
        # (Should that selection leave fewer than two segments there, every query is kept instead.)
        det = model.detections(batches[1])
        labels = det["labels"].cpu().numpy()
        h, w = ORIGINAL[1][0]
        for thr, stuff in ((float(np.median(det["scores"].cpu().numpy())), (int(np.bincount(labels.reshape(-1)).argmax()),)), (0.0, ())):
            seg = model.panoptic_segmentation(batches[1], score_threshold=thr, min_area=MIN_AREA, stuff_classes=stuff)
            ids = seg["panoptic_ids"][0].cpu().numpy()[:h, :w]
            area = seg["segment_area"][0].cpu().numpy()
            pick = [int(n) for n in np.argsort(-area) if 0 < area[n] < h * w][:2]
            if len(pick) == 2:
                break
        assert len(pick) == 2, area.tolist()
        records[1][0]["segmentation"] = [{"size": [h, w], "counts": RR.mask_to_counts(ids == n)} for n in pick]
        records[1][0]["iscrowd"] = [0, 0]
        _attach(batches[1], records[1])
        batches[1]["category"][0, :2] = seg["segment_label"][0, pick]
        torch.cuda.synchronize()
        yield batches, records, model, thr, stuff
    finally:
        K.set_deterministic(prev)


def test_evaluate_panoptic_end_to_end(trained):
    from boosted_detr_amd.evaluation import PanopticEvaluator
    from test_coco_eval_gpu import exactly, state_of
    from test_mask_image_eval_gpu import ORIGINAL
    batches, records, model, thr, stuff = trained
    Cn, both = model.num_categories, ("bbox", "segm")
    model.predict_raw(batches[0])                    # the user's last call
    users_masks = model.panoptic_masks().clone()
    ap_before = model.evaluate(batches, coco=True, iou_types=both, mask_resolution="image")
    before = state_of(model)
    ev = PanopticEvaluator(Cn, score_threshold=thr, min_area=MIN_AREA, stuff_classes=stuff)
    res = model.evaluate_panoptic(batches, evaluator=ev)
    by_keywords = model.evaluate_panoptic(batches, score_threshold=thr, min_area=MIN_AREA, stuff_classes=stuff, return_dict=False)
    torch.cuda.synchronize()
    after = state_of(model)
    assert before[1] == after[1] and set(before[0]) == set(after[0]) and len(before[0]) > 100
    for k, t in before[0].items():
        assert torch.equal(t, after[0][k]), k        # weights, moving statistics, optimizer slots: bit-identical
    assert torch.equal(model.panoptic_masks(), users_masks)
    ap_after = model.evaluate(batches, coco=True, iou_types=both, mask_resolution="image")
    assert set(ap_before) == set(ap_after)
    assert all(exactly(a, b) for a, b in zip(list(ap_before["stats"]) + list(ap_before["mask_stats"]), list(ap_after["stats"]) + list(ap_after["mask_stats"])))
    assert by_keywords == [res["PQ"], res["SQ"], res["RQ"]]

    # the reference: predict_raw / panoptic_masks() through the NumPy rules, the segmentations through the plain-loop rasteriser
    is_stuff = np.zeros(Cn, np.uint8)
    is_stuff[list(stuff)] = 1
    images = []
    for i, b in enumerate(batches):
        cat, _, _ = model.predict_raw(b)
        logits = model.panoptic_masks().cpu().numpy().reshape(2, 30, 23, 23)
        score, label = R.postprocess(cat.cpu().numpy())
        gt_label, nobj = b["category"].cpu().numpy(), b["num_objects"].cpu().numpy()
        for k, (h, w) in enumerate(ORIGINAL[i]):
            segs = records[i][k]["segmentation"] + [None] * (5 - len(records[i][k]["segmentation"]))
            masks = np.stack([RR.segmentation_mask(s, h, w) for s in segs])
            images.append(P.image_reference(logits[k], score[k], label[k], is_stuff, thr, masks, gt_label[k], np.asarray(b["iscrowd"])[k],
                                            int(nobj[k]), Cn, MIN_AREA, h, w))
    model.predict_raw(batches[0])
    rec = ev._to_host()
    for i, im in enumerate(images):
        for k, key in enumerate(("gt_state", "pred_state", "match_inter", "match_union", "gt_label", "pred_label")):
            assert np.array_equal(rec[i // 2][k][i % 2], im[key]), (i, key, rec[i // 2][k][i % 2].tolist(), im[key].tolist())
    want = P.pq(images, Cn, stuff)
    assert res["tp"].tolist() == want["tp"] and res["fp"].tolist() == want["fp"] and res["fn"].tolist() == want["fn"]
    for s in ("", "_th", "_st"):
        assert all(abs(res[k + s] - want[k + s]) <= 1e-12 for k in ("PQ", "SQ", "RQ")), (s, res, want)
        assert res["num_classes_scored" + s] == want["num_classes_scored" + s]
    assert res["num_images"] == 4 and sum(want["tp"]) >= 2 and res["PQ"] > 0.0 and sum(want["fn"]) > 0
    assert any((im["seg_of"] >= 0).sum() >= 5 for im in images)

    it = model.optimizer.iterations                  # and training goes on as if nothing had happened
    logs = model.logs_to_host(model.train_step(batches[0]))
    assert math.isfinite(logs["loss"]) and model.optimizer.iterations == it + 1


def test_panoptic_segmentation(trained):
    from test_mask_image_eval_gpu import ORIGINAL
    batches, _, model, thr, stuff = trained
    for i, b in enumerate(batches):
        seg = model.panoptic_segmentation(b, score_threshold=thr, min_area=MIN_AREA, stuff_classes=stuff)
        assert set(seg) == {"panoptic_ids", "segment_label", "segment_score", "segment_area", "image_hw"}
        Hm, Wm = MI.layout(ORIGINAL[i])
        ids, area = seg["panoptic_ids"], seg["segment_area"]
        assert ids.dtype == torch.int16 and tuple(ids.shape) == (2, Hm, 64 * Wm) and area.dtype == torch.int32 and tuple(area.shape) == (2, 30)
        assert tuple(seg["segment_label"].shape) == tuple(seg["segment_score"].shape) == (2, 30)
        assert seg["image_hw"].cpu().tolist() == [list(v) for v in ORIGINAL[i]]
        ids, area = ids.cpu().numpy(), area.cpu().numpy()
        score, label = seg["segment_score"].cpu().numpy(), seg["segment_label"].cpu().numpy()
        for k, (h, w) in enumerate(ORIGINAL[i]):
            inside = np.zeros(ids[k].shape, bool)
            inside[:h, :w] = True
            assert (ids[k][~inside] == -1).all()
            counts = np.bincount(ids[k][ids[k] >= 0].astype(np.int64), minlength=30)
            assert np.array_equal(counts, area[k]), (i, k, counts.tolist(), area[k].tolist())
            assert all(a == 0 or a >= MIN_AREA for a in area[k]) and all(score[k, n] > np.float32(thr) for n in np.flatnonzero(area[k]))
            # with min_area 0 and no stuff the map is the reference's merge of the kept queries, and some segment was dropped above
            full = model.panoptic_segmentation(b, score_threshold=thr, min_area=0)
            logits = model.panoptic_masks().cpu().numpy().reshape(2, 30, 23, 23)
            want = P.merge(logits[k], P.select(score[k], label[k], None, thr), h, w)
            assert np.array_equal(full["panoptic_ids"][k].cpu().numpy(), P.ids_canvas(want, Hm, Wm))
            assert np.array_equal(full["segment_area"][k].cpu().numpy(), np.bincount(want[want >= 0], minlength=30))


def test_callback_logs_the_three_keys(trained):
    from boosted_detr_amd.training import PanopticQuality
    batches, _, model, thr, stuff = trained
    cb = PanopticQuality(batches, score_threshold=thr, min_area=MIN_AREA, stuff_classes=stuff)
    cb.set_model(model)
    logs = {}
    cb.on_epoch_end(0, logs)
    want = model.evaluate_panoptic(batches, score_threshold=thr, min_area=MIN_AREA, stuff_classes=stuff)
    assert logs == {"val_PQ": want["PQ"], "val_SQ": want["SQ"], "val_RQ": want["RQ"]} and cb.history[0]["epoch"] == 0
    every = PanopticQuality(batches, every=2)
    every.set_model(model)
    logs = {}
    every.on_epoch_end(0, logs)
    assert logs == {} and every.history == []


def test_refusals(trained):
    from boosted_detr_amd.boosted_model import BoostedDETR
    from boosted_detr_amd.evaluation import PanopticEvaluator, host_image_hw
    from boosted_detr_amd.model import DETR
    batches, _, model, thr, stuff = trained
    boosted, plain = object.__new__(BoostedDETR), object.__new__(DETR)
    plain.__dict__["PanopticAttention"] = None       # what DETR() without with_panoptic_head leaves
    for m, match in ((boosted, "BoostedDETR has no mask head"), (plain, "with_panoptic_head=True")):
        with pytest.raises(RuntimeError, match=match):
            m.evaluate_panoptic(batches)
        with pytest.raises(RuntimeError, match=match):
            m.panoptic_segmentation(batches[0])
    # a batch over max_mask_bytes is refused before any launch, and the evaluator stays usable
    Cn = model.num_categories
    hw0, hw1 = (host_image_hw(b["height"], b["width"]) for b in batches)
    need = [8 * int(hw[:, 0].max()) * ((int(hw[:, 1].max()) + 63) // 64) * 2 * (30 + 5) for hw in (hw0, hw1)]
    assert need[0] > need[1]
    ev = PanopticEvaluator(Cn, score_threshold=thr, min_area=MIN_AREA, stuff_classes=stuff, max_mask_bytes=need[1])
    with pytest.raises(ValueError, match="max_mask_bytes"):
        model.evaluate_panoptic(batches, evaluator=ev)
    assert ev._kept == [] and ev.last is None
    got = model.evaluate_panoptic(batches[1:], evaluator=ev)
    want = model.evaluate_panoptic(batches[1:], score_threshold=thr, min_area=MIN_AREA, stuff_classes=stuff)
    assert got["num_images"] == 2 and all(got[k] == want[k] for k in ("PQ", "SQ", "RQ")) and got["tp"].tolist() == want["tp"].tolist()
