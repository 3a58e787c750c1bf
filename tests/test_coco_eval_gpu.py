"""GPU half of the full COCO protocol: bdetr_det_match_coco (K16) and bdetr_mask_match_coco (K17) against the plain-loop reference
(tests/_coco_ref.py), bit for bit (order, class_rank, tp_bits, ig_bits, matched_gt, gt_count), against K14 / K15 where the protocols
coincide, and Model.evaluate(coco=True) / DetectionAP(coco=True) end to end."""
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import _coco_cases as CS
import _coco_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def as_logits(mask):
    return np.where(mask, 1.5, -1.5).astype(np.float32)


def to_host(order, class_rank, tp_bits, ig_bits, matched):
    torch.cuda.synchronize()
    return (order.cpu().numpy(), class_rank.cpu().numpy(), tp_bits.cpu().numpy().view(np.uint16), ig_bits.cpu().numpy().view(np.uint16),
            matched.cpu().numpy())


def run_box(c, gt_count=None):
    from boosted_detr_amd import kernels as K
    A = len(c["area_ranges"])
    if gt_count is None:
        gt_count = torch.zeros(A, c["C"], dtype=torch.int32, device=DEV)
    out = K.det_match_coco(dev(c["score"]), dev(c["label"]), dev(c["box"]), dev(c["gt_label"]), dev(c["gt_box"]), dev(c["gt_crowd"]),
                           None if c["gt_area"] is None else dev(c["gt_area"]), dev(c["num_objects"]), dev(c["image_hw"]), dev(c["area_ranges"]),
                           c["thresholds"], c["C"], c["max_dets"], gt_count)
    return to_host(*out) + (gt_count,)


def run_mask(c, gt_count=None):
    from boosted_detr_amd import kernels as K
    A = len(c["area_ranges"])
    if gt_count is None:
        gt_count = torch.zeros(A, c["C"], dtype=torch.int32, device=DEV)
    det_bits, det_pop = K.mask_binarize(dev(as_logits(c["mask"])), 0.0)
    gt_bits, gt_pop = K.mask_binarize(dev(c["gt_mask"].astype(np.float32)), 0.5)
    out = K.mask_match_coco(dev(c["score"]), dev(c["label"]), det_bits, det_pop, dev(c["gt_label"]), gt_bits, gt_pop, dev(c["gt_crowd"]),
                            None if c["gt_area"] is None else dev(c["gt_area"]), dev(c["num_objects"]), dev(c["image_hw"]), dev(c["area_ranges"]),
                            c["thresholds"], c["mask"].shape[-1], c["C"], c["max_dets"], gt_count)
    return to_host(*out) + (gt_count,)


def assert_bit_exact(name, images, got):
    order, class_rank, tp_bits, ig_bits, matched, gt_count = got
    A = images[0]["tp"].shape[0]
    for b, im in enumerate(images):
        assert np.array_equal(order[b], im["order"]), (name, b, "order")
        assert np.array_equal(class_rank[b], im["class_rank"]), (name, b, "class_rank")
        for a in range(A):
            assert np.array_equal(tp_bits[a, b], R.pack_bits(im["keep"], im["tp"][a])), (name, a, b, "tp_bits")
            assert np.array_equal(ig_bits[a, b], R.pack_bits(im["keep"], im["ig"][a], with_keep=False)), (name, a, b, "ig_bits")
            assert np.array_equal(matched[a, b], im["matched_gt"][a]), (name, a, b, "matched_gt")
    assert np.array_equal(gt_count.cpu().numpy(), sum(im["gt_count"] for im in images)), (name, "gt_count")
    assert not (tp_bits & ig_bits & 0x7FFF).any()                      # tp and ig are mutually exclusive


# ---------------------------------------------------------------------------------------------------------------------
# 6. bit-exact against the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CS.BOX_CASES))
def test_box_match_bit_exact(cuda, name):
    c, images = CS.BOX_CASES[name], CS.reference(name)
    got = run_box(c)
    assert_bit_exact(name, images, got)
    order, class_rank, tp_bits, ig_bits, matched, gt_count = got
    counts = gt_count.cpu().numpy()
    counters = {k: sum(im["counters"][k] for im in images) for k in images[0]["counters"]}
    # each case exercises what it is there for (properties of the reference's answer, so of the kernel's too)
    if name == "crowd_N100_M130":
        assert c["gt_label"].shape[1] > 128 and counters["crowd_rematch"][0] > 0 and counters["preferred_over_better_ignored"][0] > 0
        assert (counts.sum(1) > 0).all() and (tp_bits & 0x3FF).any() and (ig_bits != 0).any()
    if name == "B3_N50_M20":
        assert counts[3].sum() == 0 and counts[0].sum() == 27 and (matched[:, 0] == -1).all() and (ig_bits[0] == 0).all()      # "large" is empty
    if name == "duplicated_scores":
        assert len(np.unique(c["score"])) == 4 and counters["crowd_rematch"][0] > 0
    if name == "duplicated_gt_one_of_each_pair_crowd":
        # exactly on a pair: the non-ignored twin is taken whichever row it has, with IoU 1 at every threshold
        assert (matched[0, 0, :, :6] == np.arange(1, 12, 2)).all() and (matched[0, 1, :, :6] == np.arange(0, 12, 2)).all()
        assert ((tp_bits[0, :, :6] & 0x3FF) == 0x3FF).all()
    if name == "padding_rows_flagged_crowd":
        assert (matched[:, 0] < 4).all() and (matched[:, 1] == -1).all() and counts[0].sum() == 4 and counters["crowd_rematch"].sum() == 0
    if name == "one_class_all_crowd":
        assert (counts[:, 3] == 0).all() and counts[0].sum() > 0 and ((tp_bits[:, c["label"] == 3] & 0x3FF) == 0).all()
        assert (ig_bits[0][c["label"] == 3] != 0).any()
    if name == "gt_area_contradicts_box":
        assert not np.array_equal(counts[1:], sum(im["gt_count"] for im in CS.reference("gt_area_null"))[1:])
        assert counts[2].sum() == 0 and counts[1].sum() > 0 and counts[3].sum() > 0      # 500 is small, 20000 is large, nothing is medium


@pytest.mark.parametrize("name", list(CS.MASK_CASES))
def test_mask_match_bit_exact(cuda, name):
    c, images = CS.MASK_CASES[name], CS.reference(name)
    got = run_mask(c)
    assert_bit_exact(name, images, got)
    counts = got[5].cpu().numpy()
    counters = {k: sum(im["counters"][k] for im in images) for k in images[0]["counters"]}
    assert counters["crowd_rematch"][0] > 0 and counters["unmatched_out_of_range"].sum() > 0 and (got[2] & 0x3FF).any() and got[3].any()
    if name == "P529_B2_N60_M70":
        assert c["mask"].shape[-1] == 529 and (counts.sum(1) > 0).all()
    else:
        assert c["mask"].shape[-1] == 70
    if name == "P70_gt_area_given":
        assert not np.array_equal(counts, sum(im["gt_count"] for im in CS.reference("P70_B2_N37_M12")))


# ---------------------------------------------------------------------------------------------------------------------
# 7. no crowd, range "all": K16 is K14 and K17 is K15
# ---------------------------------------------------------------------------------------------------------------------
def test_box_equals_k14_without_crowd_and_ranges(cuda):
    from boosted_detr_amd import kernels as K
    for c in (CS.make_case(1, 3, 50, 20, 8, [0, 20, 7]), CS.make_case(3, 1, 300, 100, 8, [100], crowded_class=3),
              CS.make_case(4, 2, 50, 20, 5, [20, 11], score_levels=[0.125, 0.25, 0.5, 0.7])):
        old_count = torch.zeros(c["C"], dtype=torch.int32, device=DEV)
        o_order, o_bits, o_matched = K.det_match(dev(c["score"]), dev(c["label"]), dev(c["box"]), dev(c["gt_label"]), dev(c["gt_box"]),
                                                 dev(c["num_objects"]), c["thresholds"], c["C"], 100, old_count)
        order, class_rank, tp_bits, ig_bits, matched, gt_count = run_box(CS.coco_fields(c, (480, 640), ranges=CS.ALL_ONLY))
        assert torch.equal(o_order.cpu(), torch.from_numpy(order)) and np.array_equal(o_bits.cpu().numpy().view(np.uint16), tp_bits[0])
        assert np.array_equal(o_matched.cpu().numpy(), matched[0]) and (ig_bits[0] == 0).all()
        assert np.array_equal(old_count.cpu().numpy(), gt_count.cpu().numpy()[0])
        assert ((class_rank < 100) == ((tp_bits[0] & 0x8000) != 0)).all() and (tp_bits[0] & 0x3FF).any()


def test_mask_equals_k15_without_crowd_and_ranges(cuda):
    from boosted_detr_amd import kernels as K
    for grid, seed in (((23, 23), 31), ((5, 14), 32)):
        c = CS.make_mask_case(seed, 2, 40, 30, grid, 5, [30, 17], (480, 640), crowd_fraction=0.0)
        c["area_ranges"] = CS.ALL_ONLY
        det_bits, det_pop = K.mask_binarize(dev(as_logits(c["mask"])), 0.0)
        gt_bits, gt_pop = K.mask_binarize(dev(c["gt_mask"].astype(np.float32)), 0.5)
        old_count = torch.zeros(c["C"], dtype=torch.int32, device=DEV)
        o_order, o_bits, o_matched = K.mask_match(dev(c["score"]), dev(c["label"]), det_bits, det_pop, dev(c["gt_label"]), gt_bits, gt_pop,
                                                  dev(c["num_objects"]), c["thresholds"], c["C"], 100, old_count)
        order, class_rank, tp_bits, ig_bits, matched, gt_count = run_mask(c)
        assert np.array_equal(o_order.cpu().numpy(), order) and np.array_equal(o_bits.cpu().numpy().view(np.uint16), tp_bits[0])
        assert np.array_equal(o_matched.cpu().numpy(), matched[0]) and (ig_bits[0] == 0).all() and (tp_bits[0] & 0x3FF).any()
        assert np.array_equal(old_count.cpu().numpy(), gt_count.cpu().numpy()[0])


# ---------------------------------------------------------------------------------------------------------------------
# 8. plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_gt_count_accumulates_across_calls(cuda):
    c = CS.BOX_CASES["off_wave_N37_M5"]
    gt_count = run_box(c)[5]
    once = gt_count.cpu().numpy().copy()
    run_box(c, gt_count)
    assert np.array_equal(gt_count.cpu().numpy(), 2 * once) and once[0].sum() > 0 and once.shape == (4, 6)
    m = CS.MASK_CASES["P70_B2_N37_M12"]
    gt_count = run_mask(m)[5]
    once = gt_count.cpu().numpy().copy()
    run_mask(m, gt_count)
    assert np.array_equal(gt_count.cpu().numpy(), 2 * once) and once[0].sum() > 0


def raw_call(masks, N=8, M=4, T=3, C=5, A=2, P=70):
    """The C entry points on sentinel-filled outputs -> (status, message, outputs)."""
    from boosted_detr_amd import _lib
    W = (P + 63) // 64
    score, label = torch.rand(1, N, device=DEV), torch.full((1, N), 2, dtype=torch.int32, device=DEV)
    gl = torch.full((1, M), 2, dtype=torch.int32, device=DEV)
    crowd = torch.zeros(1, M, dtype=torch.uint8, device=DEV)
    nobj = torch.full((1,), M, dtype=torch.int32, device=DEV)
    hw = torch.tensor([[480, 640]], dtype=torch.int32, device=DEV)
    Aa, Tt = max(A, 1), max(T, 1)
    ranges = torch.tensor([[0.0, 1e10]] * Aa, dtype=torch.float64, device=DEV)
    outs = [torch.full((1, N), -7, dtype=torch.int32, device=DEV), torch.full((1, N), -7, dtype=torch.int32, device=DEV),
            torch.full((Aa, 1, N), -7, dtype=torch.int16, device=DEV), torch.full((Aa, 1, N), -7, dtype=torch.int16, device=DEV),
            torch.full((Aa, 1, Tt, N), -7, dtype=torch.int32, device=DEV)]
    count = torch.zeros(Aa, max(C, 3), dtype=torch.int32, device=DEV)
    thr = np.linspace(0.5, 0.95, Tt)
    stream = torch.cuda.current_stream().cuda_stream
    if masks:
        db, dp = torch.zeros(1, N, W, dtype=torch.int64, device=DEV), torch.zeros(1, N, dtype=torch.int32, device=DEV)
        gb, gp = torch.zeros(1, M, W, dtype=torch.int64, device=DEV), torch.zeros(1, M, dtype=torch.int32, device=DEV)
        st = _lib.lib().bdetr_mask_match_coco(score.data_ptr(), label.data_ptr(), db.data_ptr(), dp.data_ptr(), gl.data_ptr(), gb.data_ptr(),
                                              gp.data_ptr(), crowd.data_ptr(), None, nobj.data_ptr(), hw.data_ptr(), ranges.data_ptr(),
                                              thr.ctypes.data, 1, N, M, P, C, T, A, 100, *[o.data_ptr() for o in outs], count.data_ptr(), stream)
    else:
        box, gb = torch.rand(1, N, 4, device=DEV), torch.rand(1, M, 4, device=DEV)
        st = _lib.lib().bdetr_det_match_coco(score.data_ptr(), label.data_ptr(), box.data_ptr(), gl.data_ptr(), gb.data_ptr(), crowd.data_ptr(),
                                             None, nobj.data_ptr(), hw.data_ptr(), ranges.data_ptr(), thr.ctypes.data, 1, N, M, C, T, A, 100,
                                             *[o.data_ptr() for o in outs], count.data_ptr(), stream)
    msg = _lib.lib().bdetr_last_error() if st != 0 else b""
    torch.cuda.synchronize()
    return st, msg, outs + [count]


@pytest.mark.parametrize("masks", [False, True], ids=["box", "mask"])
@pytest.mark.parametrize("over", [dict(A=0), dict(A=5), dict(N=1025), dict(M=1025), dict(T=16), dict(T=0), dict(C=2)])
def test_over_limit_shapes_are_refused_without_a_launch(cuda, masks, over):
    from boosted_detr_amd import _lib
    st, msg, outs = raw_call(masks, **over)
    assert st == -1 and (b"bdetr_mask_match_coco" if masks else b"bdetr_det_match_coco") in msg
    assert all((o == -7).all() for o in outs[:5]) and (outs[5] == 0).all()      # nothing ran
    with pytest.raises(_lib.BdetrError):
        _lib.check(st, "match_coco")


def test_mask_lds_overrun_is_refused_and_the_call_itself_works(cuda):
    st, msg, outs = raw_call(True, N=100, M=100, P=39 * 64)      # 3400 + 8 * 39 * 200 = 65800 > 65536
    assert st == -1 and b"bdetr_mask_match_coco" in msg and b"LDS" in msg and b"65536" in msg
    assert all((o == -7).all() for o in outs[:5]) and (outs[5] == 0).all()
    st, msg, outs = raw_call(True, N=1024, M=1024, P=64 * 4)
    assert st == -1 and b"LDS" in msg
    for masks in (False, True):                                    # the same call inside the limits runs
        st, _, outs = raw_call(masks)
        assert st == 0 and not any((o == -7).any() for o in outs[:5]) and outs[5][:, 2].tolist() == [4, 4]


def test_largest_shapes_run(cuda):
    """Boxes at N = M = 1024, T = 15, A = 4 (59 KiB of LDS): with no crowd, range 0 = "all" must be K14's answer on the same inputs.
    Masks at N = M = 100 with W = 38 words (3400 + 60800 = 64200 bytes; W = 39 is refused above) against the reference."""
    from boosted_detr_amd import kernels as K
    c = CS.make_case(12, 1, 1024, 1024, 40, [1024])
    c["thresholds"] = np.linspace(0.3, 1.0, 15)
    old_count = torch.zeros(c["C"], dtype=torch.int32, device=DEV)
    o_order, o_bits, o_matched = K.det_match(dev(c["score"]), dev(c["label"]), dev(c["box"]), dev(c["gt_label"]), dev(c["gt_box"]),
                                             dev(c["num_objects"]), c["thresholds"], c["C"], 100, old_count)
    rng = np.random.default_rng(5)
    for crowd in (None, rng.random((1, 1024)) < 0.2):
        order, class_rank, tp_bits, ig_bits, matched, gt_count = run_box(CS.coco_fields(c, (480, 640), crowd))
        assert np.array_equal(o_order.cpu().numpy(), order) and not (tp_bits & ig_bits & 0x7FFF).any()
        assert (np.sort(order[0]) == np.arange(1024)).all() and ((tp_bits & 0x8000) != 0).all() and (tp_bits & 0x1).any()
        if crowd is None:
            assert np.array_equal(o_bits.cpu().numpy().view(np.uint16), tp_bits[0]) and np.array_equal(o_matched.cpu().numpy(), matched[0])
            assert (ig_bits[0] == 0).all() and np.array_equal(old_count.cpu().numpy(), gt_count.cpu().numpy()[0])
        else:
            m0 = matched[0, 0]                                                                     # range "all", the image: [T,N]
            assert crowd[0][m0[m0 >= 0]].any() and (ig_bits[0] != 0).any()                      # crowd regions are matched, and ignored
            taken_real = m0[0][(m0[0] >= 0) & ~crowd[0][np.maximum(m0[0], 0)]]
            assert len(taken_real) > 0 and len(np.unique(taken_real)) == len(taken_real)           # a non-crowd ground truth is taken once
    m = CS.make_mask_case(13, 1, 100, 100, (38, 64), 4, [100], (480, 640))
    assert m["mask"].shape[-1] == 38 * 64
    got = run_mask(m)
    im = R.match_image(m["score"][0], m["label"][0], m["mask"][0], m["gt_label"][0], m["gt_mask"][0], m["gt_crowd"][0], None, 100, 480, 640,
                       m["thresholds"], m["area_ranges"], 100, 4, R.mask_iou, R.mask_area)
    assert_bit_exact("mask_W38", [im], got)
    assert im["tp"].any() and im["ig"].any()


def test_known_answers_through_the_kernels(cuda):
    """The hand-derived cases of tests/golden/coco_eval_kats.json through CocoEvaluator.update / result."""
    from boosted_detr_amd.evaluation import CocoEvaluator
    for case in json.loads((Path(__file__).parent / "golden" / "coco_eval_kats.json").read_text())["cases"]:
        C, exp, T = case["num_classes"], case["expected"], len(case["thresholds"])
        ev = CocoEvaluator(C, case["thresholds"], case["max_dets"], dict(zip(case["area_names"], case["area_ranges"])))
        for i, im in enumerate(case["images"]):
            cat_pred = np.zeros((1, len(im["score"]), C), np.float32)
            cat_pred[0, np.arange(len(im["score"])), im["label"]] = im["score"]
            ev.update(dev(cat_pred), torch.tensor([im["box"]], dtype=torch.float32).cuda(), torch.tensor([im["gt_label"]], dtype=torch.int32).cuda(),
                      torch.tensor([im["gt_box"]], dtype=torch.float32).cuda(), torch.tensor([im["num_objects"]], dtype=torch.int32).cuda(),
                      iscrowd=torch.tensor([im["gt_crowd"]]), area=None if im["gt_area"] is None else torch.tensor([im["gt_area"]]),
                      image_hw=(im["height"], im["width"]))
            assert ev.last_matched_gt[:, 0].cpu().tolist() == exp["matched_gt"][i], case["name"]
            tp = ev._kept[-1][3].cpu().numpy().view(np.uint16)[:, 0]
            ig = ev._kept[-1][4].cpu().numpy().view(np.uint16)[:, 0]
            assert [[[int(b >> t) & 1 for b in row] for t in range(T)] for row in tp] == exp["tp"][i], case["name"]
            assert [[[int(b >> t) & 1 for b in row] for t in range(T)] for row in ig] == exp["ig"][i], case["name"]
        res = ev.result()
        for k, want in list(exp["metrics"].items()) + list(enumerate(exp["stats"])):
            got = res["stats"][k] if isinstance(k, int) else res[k]
            assert (math.isnan(got) if want is None else abs(got - want) <= 1e-12), (case["name"], k, got, want)
        assert res["gt_count_per_range"].tolist() == exp["gt_count"]


# ---------------------------------------------------------------------------------------------------------------------
# 9. end to end: the small head model of test_panoptic_train_gpu.py (64 x 64 images, 30 queries, 2 decoder blocks)
# ---------------------------------------------------------------------------------------------------------------------
STAT_KEYS = ("AP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR_1", "AR_10", "AR_100", "AR_small", "AR_medium", "AR_large")
EVAL_KEYS = ("iscrowd", "area", "height", "width")


def state_of(model):
    opt = model.optimizer
    tensors = {v.name: v.value.detach().clone() for v in model.variables}
    tensors.update({f"slot/{k}": t.detach().clone() for k, t in opt.flat_slots.items()})
    return tensors, (opt.iterations, model.steps_done, model._step_seed(), len(model._graphs), len(model.trainable_variables))


def exactly(got, want):
    return got == want or (math.isnan(got) and math.isnan(want))


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
        # a briefly trained model finds nothing: make the two objects of the second batch's first image the model's own
        # segmentations, one of them a crowd region
        seg = model.segmentations(batches[1])
        on = (seg["mask_logits"][0] > 0).flatten(1).sum(1)
        pick = torch.nonzero((on > 0) & (on < 529)).flatten()[:2]
        assert pick.numel() == 2, on.tolist()
        batches[1]["masks"][0, :2] = (seg["mask_logits"][0, pick] > 0).float()
        batches[1]["category"][0, :2] = seg["labels"][0, pick]
        batches[1]["bbox"][0, :2] = seg["boxes"][0, pick]
        M = batches[0]["bbox"].shape[1]
        crowd = np.zeros((2, 2, M), np.int64)                  # [batch, image, row]; num_objects = [2, 4] in both batches
        crowd[0, 0, 1], crowd[1, 0, 1], crowd[1, 1, 0] = 1, 1, 1
        crowd[:, 0, 4] = 1                                      # (a padding row's flag means nothing)
        rng = np.random.default_rng(3)
        for i, b in enumerate(batches):       # host arrays and device tensors are both accepted
            b["iscrowd"] = crowd[i] if i == 0 else torch.from_numpy(crowd[i]).cuda()
            b["area"] = rng.choice([400.0, 3000.0, 50000.0], (2, M)).astype(np.float32)
            b["height"], b["width"] = np.asarray([480, 333], np.int32), torch.tensor([640, 500], dtype=torch.int32)
        torch.cuda.synchronize()
        yield batches, model
    finally:
        K.set_deterministic(prev)


def test_evaluate_coco_end_to_end(trained):
    from boosted_detr_amd.evaluation import CocoEvaluator, CocoMaskEvaluator
    batches, model = trained
    C = model.num_categories
    bare = [{k: v for k, v in b.items() if k not in EVAL_KEYS} for b in batches]
    model.predict_raw(batches[0])                            # the user's last call
    users_masks = model.panoptic_masks().clone()
    before = state_of(model)
    plain = model.evaluate(batches)                          # the default path reads none of the new keys
    plain_both = model.evaluate(bare, iou_types=("bbox", "segm"))
    box_ev, mask_ev = CocoEvaluator(C), CocoMaskEvaluator(C)
    res = model.evaluate(batches, coco=True, iou_types=("bbox", "segm"), evaluator=box_ev, mask_evaluator=mask_ev)
    box_only = model.evaluate(batches, coco=True)
    by_class = model.evaluate(batches, evaluator=CocoEvaluator(C))              # an evaluator of the new class selects the new path
    as_list = model.evaluate(batches, coco=True, iou_types=("bbox", "segm"), return_dict=False)
    bare_coco = model.evaluate(bare, coco=True, iou_types=("bbox", "segm"))
    plain_after = model.evaluate(batches)
    torch.cuda.synchronize()
    after = state_of(model)
    assert before[1] == after[1] and set(before[0]) == set(after[0]) and len(before[0]) > 100
    for k, t in before[0].items():
        assert torch.equal(t, after[0][k]), k                # weights, moving statistics, optimizer slots: bit-identical
    assert torch.equal(model.panoptic_masks(), users_masks)  # and panoptic_masks() still answers for the user's last call

    # evaluate() is what it was, and does not know the new keys
    assert set(plain) == {"AP", "AP50", "AP75", "AR", "per_class_AP", "num_detections", "num_ground_truths", "num_images", "gt_count"}
    for k in ("AP", "AP50", "AP75", "AR"):
        assert exactly(plain[k], plain_after[k]) and exactly(plain[k], plain_both[k])
    # without crowds and size keys the protocols coincide on the four shared numbers, boxes and masks: the same matches (K16 = K14
    # bit for bit, above), so host fp64 means of the same at most T * R * C samples in [0, 1] - summed over the flattened array
    # here and axis by axis there, which moves the last bit; the bound is the one the existing end-to-end tests use for that
    for k in ("AP", "AP50", "AP75", "AR"):
        assert abs(bare_coco[k] - plain_both[k]) <= 1e-12, (k, bare_coco[k], plain_both[k])
        assert abs(bare_coco["mask_" + k] - plain_both["mask_" + k]) <= 1e-12, (k, bare_coco["mask_" + k], plain_both["mask_" + k])
    assert bare_coco["num_detections"] == plain_both["num_detections"] and bare_coco["num_ground_truths"] == plain_both["num_ground_truths"]
    assert np.array_equal(bare_coco["gt_count"], plain_both["gt_count"]) and plain["AP"] > 0.0

    # against the reference over predict_raw's outputs
    ref_box, ref_mask = [], []
    for b in batches:
        cat, _, box = model.predict_raw(b)
        logits = model.panoptic_masks()
        assert tuple(logits.shape) == (2, 30, 529)
        score, label = R.postprocess(cat.cpu().numpy())
        shared = {"score": score, "label": label, "gt_label": b["category"].cpu().numpy(), "num_objects": b["num_objects"].cpu().numpy(),
                  "gt_crowd": np.asarray(b["iscrowd"].cpu() if isinstance(b["iscrowd"], torch.Tensor) else b["iscrowd"]), "gt_area": b["area"],
                  "height": np.asarray(b["height"]), "width": b["width"].numpy()}
        ref_box.append(dict(shared, det=box.cpu().numpy(), gt=b["bbox"].cpu().numpy()))
        ref_mask.append(dict(shared, det=R.binarize(logits.cpu().numpy(), 0.0), gt=R.binarize(b["masks"].cpu().numpy().reshape(2, -1, 529), 0.5)))
    model.predict_raw(batches[0])
    for prefix, ev, ref_batches, masks in (("", box_ev, ref_box, False), ("mask_", mask_ev, ref_mask, True)):
        ref, images, _ = R.evaluate(ref_batches, CS.THR10, num_classes=C, masks=masks)
        records, gt_count = ev._to_host()                    # what the kernels left: integers, compared bit for bit
        for i, im in enumerate(images):
            score, label, class_rank, tp_bits, ig_bits, order = (r[:, i % 2] if r.ndim == 3 else r[i % 2] for r in records[i // 2])
            assert np.array_equal(order, im["order"]) and np.array_equal(class_rank, im["class_rank"]), (prefix, i)
            assert np.array_equal(label, im["label"]) and np.array_equal(score, im["score"]), (prefix, i)
            for a in range(4):
                assert np.array_equal(tp_bits[a], R.pack_bits(im["keep"], im["tp"][a])), (prefix, i, a)
                assert np.array_equal(ig_bits[a], R.pack_bits(im["keep"], im["ig"][a], with_keep=False)), (prefix, i, a)
        assert np.array_equal(gt_count, ref["gt_count"])
        assert len(res[prefix + "stats"]) == 12
        for i, k in enumerate(STAT_KEYS):
            assert exactly(res[prefix + k], ref[k]), (prefix, k, res[prefix + k], ref[k])
            assert exactly(res[prefix + "stats"][i], ref["stats"][i]) and exactly(res[prefix + "stats"][i], res[prefix + k])
        assert exactly(res[prefix + "AR"], ref["AR_100"])
        assert np.array_equal(res["per_class_" + prefix + "AP"], ref["per_class_AP"], equal_nan=True)
        assert sum(im["ig"].any() for im in images) > 0 and any(im["counters"]["crowd_rematch"].sum() + im["ig"][0].sum() > 0 for im in images)
    assert res["AP"] > 0.0 and res["mask_AP"] > 0.0 and res["num_images"] == 4 and res["num_detections"] == 4 * 30
    assert res["num_ground_truths"] == 12 - 3                # the three crowd regions are not counted
    assert not exactly(res["AP"], plain["AP"]) or not exactly(res["AR"], plain["AR"])       # the crowd regions and areas change the result

    assert all(exactly(box_only[k], res[k]) and exactly(by_class[k], res[k]) for k in STAT_KEYS) and "mask_AP" not in box_only
    assert len(as_list) == 24 and all(exactly(x, y) for x, y in zip(as_list, res["stats"] + res["mask_stats"]))
    only = model.evaluate(batches, coco=True, iou_types="segm")
    assert "AP" not in only and all(exactly(only["mask_" + k], res["mask_" + k]) for k in STAT_KEYS) and only["num_images"] == 4
    with pytest.raises(ValueError, match="CocoEvaluator"):
        from boosted_detr_amd.evaluation import DetectionEvaluator
        model.evaluate(batches, coco=True, evaluator=DetectionEvaluator(C))

    it = model.optimizer.iterations                          # and training goes on as if nothing had happened
    logs = model.logs_to_host(model.train_step(batches[0]))
    assert math.isfinite(logs["loss"]) and model.optimizer.iterations == it + 1


def test_fit_with_detection_ap_coco_logs_the_new_keys(cuda):
    from boosted_detr_amd.training import SGD, Callback, DetectionAP
    from test_panoptic_train_gpu import _small_head_batch, _small_head_model
    batch = _small_head_batch(9)
    batch["iscrowd"] = np.asarray([[0, 1, 0, 0, 0], [0, 0, 0, 0, 0]])
    model = _small_head_model()
    model.compile(optimizer=SGD(learning_rate=1e-3, momentum=.9, nesterov=True, clipnorm=.1))
    seen = []

    class Record(Callback):
        def on_epoch_end(self, epoch, logs=None):
            seen.append(dict(logs))

    cb = DetectionAP([batch], iou_types=("bbox", "segm"), coco=True)
    model.fit([batch] * 2, epochs=1, callbacks=[cb, Record()], verbose=0)
    assert len(seen) == 1 and model.optimizer.iterations == 2
    want = {f"val_{p}{k}" for p in ("", "mask_") for k in STAT_KEYS + ("AR",)}
    assert want <= set(seen[0]) and set(cb.history[0]) == {"epoch"} | want
    for k in want:                                           # 64 x 64 images: nothing is large, so those are NaN; a range may be empty
        ranged = k.endswith(("_small", "_medium", "_large"))
        assert math.isnan(seen[0][k]) if k.endswith("_large") else (0.0 <= seen[0][k] <= 1.0 or (ranged and math.isnan(seen[0][k]))), (k, seen[0][k])
    assert any(not math.isnan(seen[0][p + k]) for p in ("val_", "val_mask_") for k in ("AP_small", "AP_medium"))
    assert "loss" in seen[0] and "Mask_Loss" in seen[0]


def test_boosted_detr_evaluates_boxes_with_coco_and_refuses_segm(cuda):
    from boosted_detr_amd import parameters
    from boosted_detr_amd.boosted_model import BoostedDETR
    from boosted_detr_amd.engine import to_device
    from oracle import detr_oracle as O
    cfg = O.Config(image_size=(64, 64), num_object_preds=10, num_decoder_blocks=2, num_categories=12, num_attributes=6)
    host = O.make_batch(cfg, 2, 5, seed=9, num_objects=[2, 4])
    batch = {"image": to_device(host["image"]), "category": to_device(host["category"], torch.int32), "attribute": to_device(host["attribute"], torch.int32),
             "bbox": to_device(host["bbox"]), "num_objects": to_device(host["num_objects"], torch.int32),
             "iscrowd": np.asarray([[1, 0, 0, 0, 0], [0, 0, 0, 1, 0]]), "height": [480, 480], "width": [640, 640]}
    m = BoostedDETR(num_object_preds=10, image_size=(64, 64), num_encoder_blocks=1, num_encoder_heads=8, encoder_dim=256, num_decoder_blocks=2,
                    num_decoder_heads=8, decoder_dim=256, num_panoptic_heads=1, panoptic_dim=32, vocab_dict=parameters.synthetic_vocab(10, 4),
                    attribute_weight=1.0)
    from boosted_detr_amd.training import SGD
    m.compile(optimizer=SGD(learning_rate=1e-3, momentum=.9, nesterov=True, clipnorm=.1))
    m.train_step(batch)                                      # build-by-first-call
    res = m.evaluate([batch], coco=True)
    assert len(res["stats"]) == 12 and res["num_images"] == 2 and res["num_detections"] == 20 and res["num_ground_truths"] == 4
    assert res["gt_count_per_range"].shape == (4, 12) and 0.0 <= res["AR_100"] <= 1.0
    assert len(m.evaluate([batch], coco=True, return_dict=False)) == 12
    with pytest.raises(RuntimeError, match="with_panoptic_head=True"):
        m.evaluate([batch], coco=True, iou_types=("bbox", "segm"))
