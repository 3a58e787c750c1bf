"""GPU half of the mask metric: bdetr_mask_binarize against NumPy packing and bdetr_mask_match against the plain-loop reference
(tests/_mask_ap_ref.py), bit for bit (words, areas, order, tp_bits, matched_gt, gt_count), and Model.evaluate(iou_types=...) /
segmentations / DetectionAP end to end on the small head model of test_panoptic_train_gpu.py."""
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import _mask_ap_ref as R

pytestmark = pytest.mark.gpu

THR10 = np.linspace(0.5, 0.95, 10)


# ---------------------------------------------------------------------------------------------------------------------
# bdetr_mask_binarize
# ---------------------------------------------------------------------------------------------------------------------
def numpy_pack(mask):
    """bool [rows, P] -> uint64 [rows, ceil(P/64)], pixel p = bit p mod 64 of word p div 64."""
    rows, P = mask.shape
    W = (P + 63) // 64
    padded = np.zeros((rows, 64 * W), bool)
    padded[:, :P] = mask
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(rows, W)


def binarize_data(rows, P, thr, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(thr, 1.0, (rows, P)).astype(np.float32)
    flat = x.reshape(-1)
    special = [np.float32(thr), np.nan, np.inf, -np.inf, np.nextafter(np.float32(thr), np.float32(1)), np.nextafter(np.float32(thr), np.float32(-1))]
    where = rng.permutation(flat.size)
    for i, pos in enumerate(where[: max(len(special), flat.size // 5)]):      # a fifth of the elements (at least one of each, if they fit)
        flat[pos] = special[i % len(special)]
    if rows >= 7:
        x[0], x[1], x[2], x[3] = thr + 1.0, thr, np.nan, np.inf                     # all true; all AT the threshold (false); all NaN; all +inf
        x[4, :-1], x[4, -1] = -np.inf, thr + 0.25                                   # only the last pixel
    return x


@pytest.mark.parametrize("thr", [0.0, 0.5])
@pytest.mark.parametrize("rows", [1, 7, 300])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 529])
def test_binarize_matches_numpy_packing(cuda, P, rows, thr):
    from boosted_detr_amd import kernels as K
    x = binarize_data(rows, P, thr, seed=P * 1000 + rows)
    W = (P + 63) // 64
    bits, area = K.mask_binarize(torch.from_numpy(x).cuda(), thr)
    torch.cuda.synchronize()
    assert bits.dtype == torch.int64 and tuple(bits.shape) == (rows, W) and area.dtype == torch.int32 and tuple(area.shape) == (rows,)
    got = bits.cpu().numpy().view(np.uint64)
    want_mask = R.binarize(x, thr)
    want = numpy_pack(want_mask)
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], R.pack_words(want_mask[0]))                         # (the loop packing agrees with np.packbits)
    if P % 64:
        assert not (got[:, -1] >> np.uint64(P % 64)).any()                            # the tail word's unused bits
    assert np.array_equal(area.cpu().numpy(), want_mask.sum(1))
    assert np.array_equal(area.cpu().numpy(), [sum(bin(int(w)).count("1") for w in row) for row in got])
    if rows >= 7:
        assert area[:5].tolist() == [P, 0, 0, P, 1] and got[4, -1] == np.uint64(1) << np.uint64((P - 1) % 64)
    if x.size >= 6:
        assert np.isnan(x).any() and (x == np.float32(thr)).any()


def test_binarize_keeps_leading_dimensions(cuda):
    from boosted_detr_amd import kernels as K
    x = torch.randn(2, 3, 130, device="cuda")
    bits, area = K.mask_binarize(x, 0.0)
    assert tuple(bits.shape) == (2, 3, 3) and tuple(area.shape) == (2, 3)
    assert np.array_equal(bits.cpu().numpy().view(np.uint64).reshape(6, 3), numpy_pack(x.cpu().numpy().reshape(6, 130) > 0))


# ---------------------------------------------------------------------------------------------------------------------
# bdetr_mask_match
# ---------------------------------------------------------------------------------------------------------------------
def rect_masks(rng, n, h, w, k=3):
    """n masks, each the union of up to k random rectangles on an h x w grid -> bool [n, h*w].  Coarse: IoU ties are dense."""
    out = np.zeros((n, h, w), bool)
    for i in range(n):
        for _ in range(rng.integers(1, k + 1)):
            y0, x0 = rng.integers(0, h), rng.integers(0, w)
            out[i, y0:y0 + rng.integers(1, max(2, h // 2)), x0:x0 + rng.integers(1, max(2, w // 2))] = True
    return out.reshape(n, h * w)


def make_case(seed, B, N, M, grid, C, num_objects, max_dets=100, thresholds=THR10, crowded_class=None):
    """Ground-truth masks at random; half of the detections carry a ground truth's own mask (or that with one more rectangle),
    labelled like it, the others a random mask; scores from four levels."""
    rng = np.random.default_rng(seed)
    h, w = grid
    gt_mask = np.stack([rect_masks(rng, M, h, w) for _ in range(B)])
    gt_label = rng.integers(2, C, (B, M)).astype(np.int32)
    if crowded_class is not None:
        gt_label[:, : M // 2] = crowded_class
    src = rng.integers(0, M, (B, N))
    own = np.take_along_axis(gt_mask, src[..., None], 1)
    extra = np.stack([rect_masks(rng, N, h, w, k=1) for _ in range(B)])
    kind = rng.integers(0, 4, (B, N, 1))
    mask = np.where(kind == 0, own, np.where(kind == 1, own | extra, np.where(kind == 2, own & ~extra, np.stack([rect_masks(rng, N, h, w) for _ in range(B)]))))
    label = np.take_along_axis(gt_label, src, 1)
    label = np.where(rng.random((B, N)) < 0.2, rng.integers(2, C, (B, N)), label).astype(np.int32)
    if crowded_class is not None:
        label[:, : (2 * N) // 3] = crowded_class
    score = rng.choice([0.125, 0.25, 0.5, 0.75], (B, N)).astype(np.float32)
    return {"score": score, "label": label, "mask": mask, "gt_label": gt_label, "gt_mask": gt_mask,
            "num_objects": np.asarray(num_objects, np.int32), "C": C, "thresholds": np.asarray(thresholds, np.float64), "max_dets": max_dets}


def match_cases():
    cases = {}
    cases["B2_N5_M3_P65"] = make_case(1, 2, 5, 3, (5, 13), 5, [3, 2])
    # the head's own shape; num_objects 0 and above M; class 3 crowded so that max_dets = 20 truncates
    cases["head_shape_B3_N100_M100_P529"] = make_case(2, 3, 100, 100, (23, 23), 8, [0, 100, 150], max_dets=20, crowded_class=3)
    # one class, 65 objects: ground truth 64 is lane 0's SECOND `taken` bit; the best-scored detection sits exactly on it
    c = make_case(3, 1, 30, 65, (23, 23), 3, [65])
    c["mask"][0, 0], c["score"][0, 0] = c["gt_mask"][0, 64], 0.875
    c["mask"][0, 1], c["score"][0, 1] = c["gt_mask"][0, 64], 0.8125              # and the next one finds it taken
    cases["second_taken_bit_N30_M65_P529_C3"] = c

    c = make_case(4, 2, 37, 10, (5, 13), 5, [10, 10])                            # <PAD> / <OOV> among the real rows; empty masks on either side
    c["gt_label"][:, 0], c["gt_label"][:, 1] = 0, 1
    c["label"][:, 0], c["mask"][:, 0] = 1, c["gt_mask"][:, 1]                    # (a caller's own label 1 still finds no <OOV> ground truth)
    c["gt_mask"][:, 2], c["gt_mask"][:, 3] = False, False                        # empty ground truths
    c["mask"][:, 1:4], c["label"][:, 1:3] = False, c["gt_label"][:, 2:4]         # empty detections, two of them labelled like the empty ground truths
    c["label"][:, 4], c["mask"][:, 4] = c["gt_label"][:, 2], c["gt_mask"][:, 5]  # a non-empty detection against an empty ground truth
    cases["ignored_ids_and_empty_masks"] = c

    c = make_case(5, 2, 37, 12, (5, 13), 5, [12, 12])                            # duplicated ground truths: rows 2k and 2k+1 are the same object
    c["gt_mask"][:, 1::2], c["gt_label"][:, 1::2] = c["gt_mask"][:, 0::2], c["gt_label"][:, 0::2]
    c["gt_mask"][:, 0:12:2, 0] = True                                            # (no empty pair: IoU 1 needs pixels)
    c["gt_mask"][:, 1:12:2, 0] = True
    c["mask"][:, :6], c["label"][:, :6] = c["gt_mask"][:, 0:12:2], c["gt_label"][:, 0:12:2]      # six detections sit exactly on a pair
    c["score"][:, :6] = 0.99
    cases["duplicated_ground_truths"] = c

    c = make_case(6, 2, 37, 8, (5, 13), 4, [8, 5], thresholds=[1.0])             # T = 1, and the threshold 1.0: only exact copies match
    cases["T1_threshold_one"] = c
    cases["T15"] = make_case(7, 2, 37, 8, (5, 13), 4, [8, 5], thresholds=np.linspace(0.3, 1.0, 15))
    return cases


CASES = match_cases()
_REF = {}


def reference(name):
    """The reference's answer for a case, computed once and shared."""
    if name not in _REF:
        c = CASES[name]
        _, images = R.evaluate([{k: c[k] for k in ("score", "label", "mask", "gt_label", "gt_mask", "num_objects")}],
                               c["thresholds"], c["max_dets"], c["C"])
        _REF[name] = images
    return _REF[name]


def as_logits(mask):
    return np.where(mask, 1.5, -1.5).astype(np.float32)


def run_match(c, gt_count=None):
    from boosted_detr_amd import kernels as K
    dev = "cuda"
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ("score", "label", "gt_label", "num_objects")}
    det_bits, det_area = K.mask_binarize(torch.from_numpy(as_logits(c["mask"])).to(dev), 0.0)
    gt_bits, gt_area = K.mask_binarize(torch.from_numpy(c["gt_mask"].astype(np.float32)).to(dev), 0.5)
    if gt_count is None:
        gt_count = torch.zeros(c["C"], dtype=torch.int32, device=dev)
    order, tp_bits, matched = K.mask_match(t["score"], t["label"], det_bits, det_area, t["gt_label"], gt_bits, gt_area, t["num_objects"],
                                           c["thresholds"], c["C"], c["max_dets"], gt_count)
    torch.cuda.synchronize()
    return order.cpu().numpy(), tp_bits.cpu().numpy().view(np.uint16), matched.cpu().numpy(), gt_count


def check_case_properties(name, c, images, tp_bits, matched, want_count):
    """Each case exercises what it is there for (properties of the reference's answer, so of the kernel's too)."""
    keep = np.stack([im["keep"] for im in images])
    tp = np.stack([im["tp"] for im in images])
    assert len(np.unique(c["score"])) <= 6                                        # duplicated scores everywhere
    if name == "head_shape_B3_N100_M100_P529":
        assert (c["label"] == 3).sum(1).min() > 20 and (~keep).sum() == ((c["label"] == 3).sum(1) - 20).sum() and keep[c["label"] != 3].all()
        assert not tp[0].any() and (matched[0] == -1).all()                       # num_objects = 0
        assert tp[1].any() and tp[2].any() and want_count.sum() == 200            # num_objects = 150 is M
        assert tp[1:, 0].sum() > tp[1:, -1].sum() > 0
    else:
        assert keep.all()
    if name == "B2_N5_M3_P65":
        assert want_count.sum() == 5 and tp.any()
    if name == "second_taken_bit_N30_M65_P529_C3":
        assert (matched[0, :, 0] == 64).all() and (matched[0, :, 1] != 64).all() and (c["label"] == 2).all()
    if name == "ignored_ids_and_empty_masks":
        assert want_count[:2].sum() == 0 and want_count.sum() == 16 and not np.isin(matched, [0, 1]).any()
        assert (matched[:, :, :4] == -1).all()                                    # label 1; empty against empty (IoU 0); empty against anything
        assert (matched[:, :, 4] != 2).all() and not np.isin(matched, [2, 3]).any()   # nothing ever matches an empty ground truth
    if name == "duplicated_ground_truths":
        assert (matched[:, :, :6] == np.arange(1, 12, 2)[None, None, :]).all()    # equal IoU: the larger index of each pair
    if name == "T1_threshold_one":
        assert matched.shape[1] == 1 and tp.any() and not tp.all()
        hit = np.argwhere(tp[:, 0])
        assert all(np.array_equal(c["mask"][b, n], c["gt_mask"][b, matched[b, 0, n]]) for b, n in hit)
    if name == "T15":
        assert matched.shape[1] == 15 and (tp_bits & 0x4000).any() and tp[:, 0].sum() > tp[:, 14].sum()


@pytest.mark.parametrize("name", list(CASES))
def test_match_bit_exact(cuda, name):
    from boosted_detr_amd import kernels as K
    c, images = CASES[name], reference(name)
    order, tp_bits, matched, gt_count = run_match(c)
    want_count = sum(im["gt_count"] for im in images)
    for b, im in enumerate(images):
        assert np.array_equal(order[b], im["order"]), (name, b, "order")
        assert np.array_equal(tp_bits[b], R.pack_bits(im["keep"], im["tp"])), (name, b, "tp_bits")
        assert np.array_equal(matched[b], im["matched_gt"]), (name, b, "matched_gt")
    assert np.array_equal(gt_count.cpu().numpy(), want_count), name

    # the ranking and the truncation are det_match's on the same scores and labels
    B, N = c["score"].shape
    M = c["gt_label"].shape[1]
    dev = "cuda"
    box_order, box_bits, _ = K.det_match(torch.from_numpy(c["score"]).to(dev), torch.from_numpy(c["label"]).to(dev), torch.rand(B, N, 4, device=dev),
                                         torch.from_numpy(c["gt_label"]).to(dev), torch.rand(B, M, 4, device=dev),
                                         torch.from_numpy(c["num_objects"]).to(dev), c["thresholds"], c["C"], c["max_dets"],
                                         torch.zeros(c["C"], dtype=torch.int32, device=dev))
    assert np.array_equal(box_order.cpu().numpy(), order)
    assert np.array_equal(box_bits.cpu().numpy().view(np.uint16) & 0x8000, tp_bits & 0x8000)

    check_case_properties(name, c, images, tp_bits, matched, want_count)


def test_ties_are_dense_in_the_match_cases():
    """What the coarse data is for: among the IoUs a detection sees, exact ties and values ON a threshold are common."""
    c = CASES["head_shape_B3_N100_M100_P529"]
    ious = np.asarray([[R.mask_iou(d, g) for g in c["gt_mask"][1][:40]] for d in c["mask"][1][:40]])
    pos = ious[ious > 0]
    assert len(np.unique(pos)) < 0.7 * pos.size and np.isin(pos, [0.5, 0.75]).any()


def test_gt_count_accumulates_across_calls(cuda):
    c = CASES["B2_N5_M3_P65"]
    _, _, _, gt_count = run_match(c)
    once = gt_count.cpu().numpy().copy()
    run_match(c, gt_count)
    assert np.array_equal(gt_count.cpu().numpy(), 2 * once) and once.sum() == 5


@pytest.mark.parametrize("over", [dict(N=1025), dict(M=1025), dict(T=16), dict(T=0), dict(C=2), dict(max_dets=0), dict(W=0),
                                  dict(N=1024, M=1024, W=9), dict(N=100, M=100, W=40)])
def test_over_limit_shapes_are_refused_without_a_launch(cuda, over):
    from boosted_detr_amd import _lib
    N, M, T, C, max_dets, W = (over.get(k, v) for k, v in (("N", 8), ("M", 4), ("T", 3), ("C", 5), ("max_dets", 100), ("W", 2)))
    dev = "cuda"
    score, label = torch.rand(1, N, device=dev), torch.full((1, N), 2, dtype=torch.int32, device=dev)
    db, da = torch.zeros(1, N, max(W, 1), dtype=torch.int64, device=dev), torch.zeros(1, N, dtype=torch.int32, device=dev)
    gl = torch.full((1, M), 2, dtype=torch.int32, device=dev)
    gb, ga = torch.zeros(1, M, max(W, 1), dtype=torch.int64, device=dev), torch.zeros(1, M, dtype=torch.int32, device=dev)
    nobj = torch.full((1,), M, dtype=torch.int32, device=dev)
    order = torch.full((1, N), -7, dtype=torch.int32, device=dev)
    tpb = torch.full((1, N), -7, dtype=torch.int16, device=dev)
    matched = torch.full((1, max(T, 1), N), -7, dtype=torch.int32, device=dev)
    count = torch.zeros(max(C, 3), dtype=torch.int32, device=dev)
    thr = np.linspace(0.5, 0.95, max(T, 1))
    st = _lib.lib().bdetr_mask_match(score.data_ptr(), label.data_ptr(), db.data_ptr(), da.data_ptr(), gl.data_ptr(), gb.data_ptr(), ga.data_ptr(),
                                     nobj.data_ptr(), thr.ctypes.data, 1, N, M, W, C, T, max_dets, order.data_ptr(), tpb.data_ptr(),
                                     matched.data_ptr(), count.data_ptr(), torch.cuda.current_stream().cuda_stream)
    msg = _lib.lib().bdetr_last_error()
    assert st == -1 and b"bdetr_mask_match" in msg
    if "W" in over and W > 0:
        assert b"LDS" in msg and b"65536" in msg                                  # the budget is named
    torch.cuda.synchronize()
    assert (order == -7).all() and (tpb == -7).all() and (matched == -7).all() and (count == 0).all()      # nothing ran
    with pytest.raises(_lib.BdetrError):
        _lib.check(st, "mask_match")


def test_largest_shape_inside_the_lds_budget_runs(cuda):
    """N = M = 100 with W = 40 words needs 2904 + 64000 = 66904 > 65536 bytes and is refused above; W = 39 (2496 pixels) needs 65304."""
    c = make_case(9, 1, 100, 100, (39, 64), 4, [100])
    assert c["mask"].shape[-1] == 39 * 64
    order, tp_bits, matched, _ = run_match(c)
    im = R.match_image(c["score"][0], c["label"][0], c["mask"][0], c["gt_label"][0], c["gt_mask"][0], 100, c["thresholds"], 100, 4)
    assert np.array_equal(order[0], im["order"]) and np.array_equal(tp_bits[0], R.pack_bits(im["keep"], im["tp"]))
    assert np.array_equal(matched[0], im["matched_gt"]) and im["tp"].any()


def test_known_answers_through_the_kernels(cuda):
    """The hand-derived cases of tests/golden/mask_ap_kats.json through MaskEvaluator.update / result."""
    from boosted_detr_amd.evaluation import MaskEvaluator
    for case in json.loads((Path(__file__).parent / "golden" / "mask_ap_kats.json").read_text())["cases"]:
        C, exp = case["num_classes"], case["expected"]
        ev = MaskEvaluator(C, case["thresholds"], case["max_dets"])
        for im, want_tp, want_m in zip(case["images"], exp["tp"], exp["matched_gt"]):
            cat_pred = np.zeros((1, len(im["score"]), C), np.float32)
            cat_pred[0, np.arange(len(im["score"])), im["label"]] = im["score"]
            ev.update(torch.from_numpy(cat_pred).cuda(), torch.from_numpy(as_logits(np.asarray([im["mask"]], bool))).cuda(),
                      torch.tensor([im["gt_label"]], dtype=torch.int32).cuda(), torch.tensor([im["gt_mask"]], dtype=torch.float32).cuda(),
                      torch.tensor([im["num_objects"]], dtype=torch.int32).cuda())
            assert ev.last_matched_gt[0].cpu().tolist() == want_m, case["name"]
            bits = ev._kept[-1][2].cpu().numpy().view(np.uint16)[0]
            assert [[int(b >> t) & 1 for b in bits] for t in range(len(case["thresholds"]))] == want_tp, case["name"]
        res = ev.result()
        for k in ("AP", "AP50", "AP75", "AR"):
            want = exp[k]
            assert (math.isnan(res[k]) if want is None else abs(res[k] - want) <= 1e-12), (case["name"], k, res[k])
        assert res["gt_count"].tolist() == exp["gt_count"]


# ---------------------------------------------------------------------------------------------------------------------
# end to end: the small head model of test_panoptic_train_gpu.py (64 x 64 images, 30 queries, 2 decoder blocks)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(cuda):
    from boosted_detr_amd import kernels as K
    from boosted_detr_amd.training import SGD
    from test_panoptic_train_gpu import _small_head_batch, _small_head_model
    prev = K.set_deterministic(True)          # the reference below repeats evaluate's forward passes: they must give the same bits
    try:
        batches = [_small_head_batch(9), _small_head_batch(21)]
        model = _small_head_model()
        model.compile(optimizer=SGD(learning_rate=1e-3, momentum=.9, nesterov=True, clipnorm=.1))
        for i in range(3):
            model.train_step(batches[i % 2])
        # a briefly trained model finds nothing: make two of the second batch's objects the model's own segmentations, so that the
        # mask AP is not trivially 0
        seg = model.segmentations(batches[1])
        on = (seg["mask_logits"][0] > 0).flatten(1).sum(1)
        pick = torch.nonzero((on > 0) & (on < 529)).flatten()[:2]            # (neither empty nor full)
        assert pick.numel() == 2, on.tolist()
        batches[1]["masks"][0, :2] = (seg["mask_logits"][0, pick] > 0).float()
        batches[1]["category"][0, :2] = seg["labels"][0, pick]
        batches[1]["bbox"][0, :2] = seg["boxes"][0, pick]
        torch.cuda.synchronize()
        yield batches, model
    finally:
        K.set_deterministic(prev)


def test_evaluate_with_masks_end_to_end(trained):
    from boosted_detr_amd.evaluation import MaskEvaluator
    from test_detection_eval_gpu import state_of
    batches, model = trained
    C = model.num_categories
    model.predict_raw(batches[0])                            # the user's last call
    users_masks = model.panoptic_masks().clone()
    before = state_of(model)
    plain = model.evaluate(batches)
    mask_ev = MaskEvaluator(C)
    res = model.evaluate(batches, iou_types=("bbox", "segm"), mask_evaluator=mask_ev)
    only = model.evaluate(batches, iou_types="segm")
    as_list = model.evaluate(batches, iou_types=("segm", "bbox"), return_dict=False)
    torch.cuda.synchronize()
    after = state_of(model)
    assert before[1] == after[1] and set(before[0]) == set(after[0]) and len(before[0]) > 100
    for k, t in before[0].items():
        assert torch.equal(t, after[0][k]), k                # weights, moving statistics, optimizer slots: bit-identical
    assert torch.equal(model.panoptic_masks(), users_masks)  # and panoptic_masks() still answers for the user's last call

    mask_keys = ("mask_AP", "mask_AP50", "mask_AP75", "mask_AR")
    assert set(res) == set(plain) | set(mask_keys) | {"per_class_mask_AP"}
    for k, v in plain.items():                               # the box half is a plain evaluate()'s, exactly
        assert np.array_equal(res[k], v, equal_nan=True) if isinstance(v, np.ndarray) else (res[k] == v or (math.isnan(v) and math.isnan(res[k]))), k
    assert set(only) == set(mask_keys) | {"per_class_mask_AP", "num_detections", "num_ground_truths", "num_images", "gt_count"}
    assert all(only[k] == res[k] for k in mask_keys)
    assert as_list == [res[k] for k in ("AP", "AP50", "AP75", "AR") + mask_keys]

    ref_batches = []
    for b in batches:
        cat, _, _ = model.predict_raw(b)
        logits = model.panoptic_masks()
        assert tuple(logits.shape) == (2, 30, 529)
        score, label = R.postprocess(cat.cpu().numpy())
        ref_batches.append({"score": score, "label": label, "mask": R.binarize(logits.cpu().numpy(), 0.0), "gt_label": b["category"].cpu().numpy(),
                            "gt_mask": R.binarize(b["masks"].cpu().numpy().reshape(2, -1, 529), 0.5), "num_objects": b["num_objects"].cpu().numpy()})
    model.predict_raw(batches[0])                            # (leave the module's model as the next test expects it)
    ref, images = R.evaluate(ref_batches, THR10, 100, C)
    records, gt_count = mask_ev._to_host()                   # what the kernels left: integers, compared bit for bit
    for i, im in enumerate(images):
        rec = records[i // 2]
        assert np.array_equal(rec[3][i % 2], im["order"]) and np.array_equal(rec[2][i % 2], R.pack_bits(im["keep"], im["tp"])), i
        assert np.array_equal(rec[1][i % 2], im["label"]) and np.array_equal(rec[0][i % 2], im["score"]), i
    assert np.array_equal(gt_count, sum(im["gt_count"] for im in images))
    for k in ("AP", "AP50", "AP75", "AR"):                    # host fp64 means of the same samples, added in another order
        assert abs(res["mask_" + k] - ref[k]) <= 1e-12, (k, res["mask_" + k], ref[k])
    valid = gt_count > 0
    assert np.abs(res["per_class_mask_AP"][valid] - ref["per_class_AP"][valid]).max() <= 1e-12
    assert res["mask_AP"] > 0.0 and res["num_images"] == 4 and only["num_detections"] == 4 * 30 and only["num_ground_truths"] == 12

    it = model.optimizer.iterations                          # and training goes on as if nothing had happened
    logs = model.logs_to_host(model.train_step(batches[0]))
    assert math.isfinite(logs["loss"]) and math.isfinite(logs["Mask_Loss"]) and model.optimizer.iterations == it + 1


def test_evaluate_needs_masks_in_every_batch(trained):
    batches, model = trained
    without = {k: v for k, v in batches[1].items() if k != "masks"}
    keep = model._panoptic_inputs
    with pytest.raises(ValueError, match="masks"):
        model.evaluate([batches[0], without], iou_types=("bbox", "segm"))
    assert model._panoptic_inputs is keep                    # restored on the way out, too
    with pytest.raises(ValueError, match="masks"):
        model.evaluate([dict(without, masks=torch.zeros(2, 5, 22, 23, device="cuda"))], iou_types="segm")
    assert model.evaluate([without])["num_images"] == 2      # box AP asks for no masks
    with pytest.raises(ValueError, match="iou_types"):
        model.evaluate(batches, iou_types=("bbox", "keypoints"))


def test_segmentations(trained):
    batches, model = trained
    seg = model.segmentations(batches[0])
    det = model.detections(batches[0])
    assert set(seg) == {"scores", "labels", "boxes", "mask_logits", "masks"}
    assert all(t.is_cuda for t in seg.values())
    assert tuple(seg["mask_logits"].shape) == (2, 30, 23, 23) and seg["mask_logits"].dtype == torch.float32
    assert tuple(seg["masks"].shape) == (2, 30, 9) and seg["masks"].dtype == torch.int64
    for k in ("scores", "labels", "boxes"):
        assert torch.equal(seg[k], det[k])
    assert torch.equal(seg["mask_logits"].reshape(2, 30, 529), model.panoptic_masks())
    want = numpy_pack(seg["mask_logits"].cpu().numpy().reshape(60, 529) > 0)
    assert np.array_equal(seg["masks"].cpu().numpy().view(np.uint64).reshape(60, 9), want)


def test_models_without_a_mask_head_refuse_segm(cuda):
    from boosted_detr_amd import parameters
    from boosted_detr_amd.model import DETR
    plain = DETR(num_object_preds=10, image_size=(64, 64), num_encoder_blocks=1, num_encoder_heads=8, encoder_dim=256, num_decoder_blocks=1,
                 num_decoder_heads=8, decoder_dim=256, vocab_dict=parameters.synthetic_vocab(10, 4))
    with pytest.raises(RuntimeError, match="with_panoptic_head=True"):
        plain.evaluate([], iou_types=("bbox", "segm"))
    with pytest.raises(RuntimeError, match="with_panoptic_head=True"):
        plain.segmentations({})


def test_fit_with_detection_ap_logs_mask_keys(cuda):
    from boosted_detr_amd.training import SGD, Callback, DetectionAP
    from test_panoptic_train_gpu import _small_head_batch, _small_head_model
    batch = _small_head_batch(9)
    model = _small_head_model()
    model.compile(optimizer=SGD(learning_rate=1e-3, momentum=.9, nesterov=True, clipnorm=.1))
    seen = []

    class Record(Callback):
        def on_epoch_end(self, epoch, logs=None):
            seen.append(dict(logs))

    cb = DetectionAP([batch], iou_types=("bbox", "segm"))
    model.fit([batch] * 2, epochs=1, callbacks=[cb, Record()], verbose=0)
    assert len(seen) == 1 and model.optimizer.iterations == 2
    for k in ("val_AP", "val_AP50", "val_AP75", "val_AR", "val_mask_AP", "val_mask_AP50", "val_mask_AP75", "val_mask_AR"):
        assert 0.0 <= seen[0][k] <= 1.0, (k, seen[0])
    assert "loss" in seen[0] and "Mask_Loss" in seen[0] and set(cb.history[0]) == {"epoch"} | {k for k in seen[0] if k.startswith("val_")}
