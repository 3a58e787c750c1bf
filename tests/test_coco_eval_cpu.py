"""Host half of the full COCO protocol (no GPU): the plain-loop reference (tests/_coco_ref.py) against the existing no-crowd
reference where the two must agree and against hand-derived known answers (tests/golden/coco_eval_kats.json); evaluation.py's
accumulate against the reference for every (range, max_det) pair; the quality of the GPU tests' main case; the new ABI symbols."""
import json
import math
import re
from pathlib import Path

import numpy as np
import pytest

import _ap_ref as OLD
import _coco_cases as CS
import _coco_ref as R

ROOT = Path(__file__).resolve().parent.parent
KATS = json.loads((ROOT / "tests" / "golden" / "coco_eval_kats.json").read_text())["cases"]
TOL = 1e-12          # the known answers write 1 for 1 / (1 + eps)


def same(got, want):
    if want is None or (isinstance(want, float) and math.isnan(want)):
        return isinstance(got, float) and math.isnan(got)
    return abs(got - want) <= TOL


def exactly(got, want):
    return got == want or (math.isnan(got) and math.isnan(want))


def records_of(images, A):
    """One batch per image, as the K16 / K17 kernels would leave it: (score, label, class_rank, tp_bits, ig_bits, order)."""
    return [(im["score"][None].astype(np.float32), np.asarray(im["label"], np.int32)[None], im["class_rank"][None].astype(np.int32),
             np.stack([R.pack_bits(im["keep"], im["tp"][a]) for a in range(A)])[:, None],
             np.stack([R.pack_bits(im["keep"], im["ig"][a], with_keep=False) for a in range(A)])[:, None],
             np.asarray(im["order"], np.int32)[None]) for im in images]


def kat_images(case):
    """The reference's matching of a known-answer case -> (images, gt_count [A,C])."""
    C, A = case["num_classes"], len(case["area_ranges"])
    images, gt_count = [], np.zeros((A, C), np.int64)
    for im in case["images"]:
        r = R.match_image(np.asarray(im["score"], np.float32), im["label"], np.asarray(im["box"], np.float32), im["gt_label"],
                          np.asarray(im["gt_box"], np.float32), im["gt_crowd"], im["gt_area"], im["num_objects"], im["height"], im["width"],
                          case["thresholds"], case["area_ranges"], max(case["max_dets"]), C)
        r.update(score=np.asarray(im["score"], np.float32), label=np.asarray(im["label"]))
        gt_count += r["gt_count"]
        images.append(r)
    return images, gt_count


# ---------------------------------------------------------------------------------------------------------------------
# 1. without crowd, with the range "all" and one max_det the protocol IS the existing metric
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recipe", ["random_B3_N50_M20", "duplicated_scores"])
def test_reduces_to_the_existing_metric(recipe):
    c = CS.make_case(1, 3, 50, 20, 8, [0, 20, 7]) if recipe == "random_B3_N50_M20" else \
        CS.make_case(4, 2, 50, 20, 5, [20, 11], score_levels=[0.125, 0.25, 0.5, 0.7])
    B = len(c["score"])
    old, old_images = OLD.evaluate([{k: c[k] for k in ("score", "label", "box", "gt_label", "gt_box", "num_objects")}], c["thresholds"], 100, c["C"])
    batch = {"score": c["score"], "label": c["label"], "det": c["box"], "gt_label": c["gt_label"], "gt": c["gt_box"], "num_objects": c["num_objects"],
             "height": [480] * B, "width": [640] * B}
    new, images, _ = R.evaluate([batch], c["thresholds"], CS.ALL_ONLY, (100,), c["C"], area_names=["all"])
    assert len(images) == len(old_images) == B
    for im, want in zip(images, old_images):
        assert np.array_equal(im["order"], want["order"]) and np.array_equal(im["keep"], want["keep"])
        assert np.array_equal(im["tp"][0], want["tp"]) and np.array_equal(im["matched_gt"][0], want["matched_gt"])
        assert not im["ig"].any()
        assert np.array_equal(im["gt_count"][0], want["gt_count"])
    for k in ("AP", "AP50", "AP75", "AR"):
        assert new[k] == old[k], (k, new[k], old[k])                        # exactly: the same samples in the same order
    assert 0.0 < new["AP"] < 1.0 and new["stats"] == [new["AP"], new["AP50"], new["AP75"], new["AR"]]


# ---------------------------------------------------------------------------------------------------------------------
# 2. hand-derived known answers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_known_answers(case):
    from boosted_detr_amd import evaluation
    exp, A = case["expected"], len(case["area_ranges"])
    images, gt_count = kat_images(case)
    for i, im in enumerate(images):                                          # the reference's matching gives the hand-derived matches
        assert im["tp"].astype(int).tolist() == exp["tp"][i], (i, im["tp"].astype(int).tolist())
        assert im["ig"].astype(int).tolist() == exp["ig"][i], (i, im["ig"].astype(int).tolist())
        assert im["matched_gt"].tolist() == exp["matched_gt"][i], (i, im["matched_gt"].tolist())
        assert not (im["tp"] & im["ig"]).any()
        if "class_rank" in exp:
            assert im["class_rank"].tolist() == exp["class_rank"][i]
    assert gt_count.tolist() == exp["gt_count"]
    precision, recall = R.accumulate(images, gt_count, case["thresholds"], case["max_dets"])
    ref = R.summarize(precision, recall, case["thresholds"], case["max_dets"], case["area_names"])
    ev = evaluation.CocoEvaluator(case["num_classes"], case["thresholds"], case["max_dets"], dict(zip(case["area_names"], case["area_ranges"])))
    got = ev.result_from(records_of(images, A), gt_count)
    for k, want in exp["metrics"].items():
        assert same(ref[k], want), ("reference", k, ref[k], want)
        assert same(got[k], want), ("evaluation", k, got[k], want)
    assert len(ref["stats"]) == len(got["stats"]) == len(exp["stats"]) == 3 + (A - 1) + len(case["max_dets"]) + (A - 1)
    for i, want in enumerate(exp["stats"]):
        assert same(ref["stats"][i], want) and same(got["stats"][i], want), (i, ref["stats"][i], got["stats"][i], want)
    assert got["gt_count"].tolist() == exp["gt_count"][0] and got["gt_count_per_range"].tolist() == exp["gt_count"]


def test_known_answers_cover_what_they_are_there_for():
    by_name = {c["name"]: c["expected"] for c in KATS}
    assert by_name["crowd_hit_twice_is_ignored"]["matched_gt"][0][0][0][:2] == [1, 1]
    assert by_name["real_at_050_crowd_at_075"]["matched_gt"][0][0] == [[0], [1]]
    assert by_name["area_exactly_1024_is_small_and_medium_and_large_is_nan"]["gt_count"][1:3] == [[0, 0, 1], [0, 0, 1]]
    assert by_name["ar_1_below_ar_10"]["metrics"]["AR_1"] < by_name["ar_1_below_ar_10"]["metrics"]["AR_10"]
    assert by_name["range_without_ground_truth_is_nan_and_class_without_joins_no_mean"]["metrics"]["AP_medium"] is None


# ---------------------------------------------------------------------------------------------------------------------
# 3. the host accumulate against the reference, every (range, max_det) pair
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["crowd_N100_M130", "B3_N50_M20", "duplicated_scores", "one_class_all_crowd"])
def test_accumulate_matches_reference_exactly(name):
    from boosted_detr_amd import evaluation
    c, images = CS.BOX_CASES[name], CS.reference(name)
    for b, im in enumerate(images):
        im.update(score=c["score"][b], label=c["label"][b])
    gt_count = sum(im["gt_count"] for im in images)
    max_dets = [1, 10, 100]
    precision, recall = R.accumulate(images, gt_count, c["thresholds"], max_dets)
    ref = R.summarize(precision, recall, c["thresholds"], max_dets)
    ev = evaluation.CocoEvaluator(c["C"], c["thresholds"], max_dets)            # constructing one needs no GPU
    assert ev.area_names == ["all", "small", "medium", "large"] and np.array_equal(ev.area_ranges, CS.COCO_RANGES) and ev.max_dets == (1, 10, 100)
    records = records_of(images, 4)
    got = ev.result_from(records, gt_count)
    assert len(got["stats"]) == 12
    for i in range(12):
        assert exactly(got["stats"][i], ref["stats"][i]), (i, got["stats"][i], ref["stats"][i])
    for k in ("AP", "AP50", "AP75", "AR", "AP_small", "AP_medium", "AP_large", "AR_1", "AR_10", "AR_100", "AR_small", "AR_medium", "AR_large"):
        assert exactly(got[k], ref[k]), (k, got[k], ref[k])
    assert np.array_equal(got["per_class_AP"], ref["per_class_AP"], equal_nan=True)
    lineup = evaluation._Lineup(records, 4)
    for a in range(4):
        for mi, m in enumerate(max_dets):                                        # also the pairs that summarize never reads
            p, r = evaluation.accumulate_pair(lineup, gt_count[a], len(c["thresholds"]), a, m)
            assert np.array_equal(p, precision[:, :, :, a, mi]) and np.array_equal(r, recall[:, :, a, mi]), (a, m)
    if name == "crowd_N100_M130":
        assert 0.0 < ref["AP"] < 1.0 and ref["AR_1"] < ref["AR_10"] <= ref["AR_100"] and not any(math.isnan(v) for v in ref["stats"])
    if name == "B3_N50_M20":
        assert math.isnan(ref["AP_large"]) and math.isnan(ref["AR_large"]) and gt_count[3].sum() == 0


def test_batched_records_and_empty_evaluator():
    from boosted_detr_amd import evaluation
    c, images = CS.BOX_CASES["B3_N50_M20"], CS.reference("B3_N50_M20")
    for b, im in enumerate(images):
        im.update(score=c["score"][b], label=c["label"][b])
    gt_count = sum(im["gt_count"] for im in images)
    ev = evaluation.CocoEvaluator(c["C"])
    recs = records_of(images, 4)
    single = ev.result_from(recs, gt_count)
    batched = [tuple(np.concatenate([r[k] for r in recs[:2]], axis=1 if k in (3, 4) else 0) for k in range(6)), recs[2]]
    both = ev.result_from(batched, gt_count)
    assert all(exactly(x, y) for x, y in zip(single["stats"], both["stats"])) and single["num_images"] == both["num_images"] == 3
    empty = evaluation.CocoEvaluator(5).result()
    assert all(math.isnan(v) for v in empty["stats"]) and len(empty["stats"]) == 12 and empty["num_detections"] == 0
    mask_ev = evaluation.CocoMaskEvaluator(5, max_dets=(10, 1), area_ranges={"all": (0, 1e10), "tiny": (0, 100)})
    assert mask_ev.max_dets == (1, 10) and mask_ev.area_names == ["all", "tiny"] and isinstance(mask_ev, evaluation.CocoEvaluator)
    assert list(k for k in mask_ev.result() if k.startswith(("AP", "AR"))) == ["AP", "AP50", "AP75", "AP_tiny", "AR_1", "AR_10", "AR_tiny", "AR"]
    for bad in (dict(area_ranges=[[0, 1]] * 5), dict(area_ranges={}), dict(max_dets=(0, 10)), dict(iou_thresholds=np.linspace(0, 1, 16))):
        with pytest.raises(ValueError):
            evaluation.CocoEvaluator(5, **bad)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the main GPU case exercises the new rules (a property of the reference's answer)
# ---------------------------------------------------------------------------------------------------------------------
def test_crowd_case_quality():
    c = CS.BOX_CASES["crowd_N100_M130"]
    assert c["score"].shape == (1, 100) and c["gt_label"].shape == (1, 130) and c["C"] == 6 and c["image_hw"].tolist() == [[480, 640]]
    assert len(c["thresholds"]) == 10 and 0.1 < c["gt_crowd"].mean() < 0.3
    im = CS.reference("crowd_N100_M130")[0]
    k = im["counters"]
    assert k["crowd_rematch"][0] > 0                                  # crowd ground truths taken while already matched
    assert k["preferred_over_better_ignored"][0] > 0                  # a non-ignored ground truth taken although an ignored one had a higher IoU
    assert k["unmatched_out_of_range"].sum() > 0                      # detections ignored for being unmatched and out of range
    assert (k["tp_out_of_range"] > 0).any()                           # TPs whose own area is out of range
    assert (im["gt_count"].sum(1) > 0).all()                          # all four ranges have npig > 0
    assert not (im["tp"] & im["ig"]).any()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the new symbols
# ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared():
    from boosted_detr_amd import _lib, build, evaluation, kernels, pipeline, training
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "bdetr.h").read_text(), flags=re.S)
    for name in ("bdetr_det_match_coco", "bdetr_mask_match_coco"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, header)
    full = (ROOT / "include" / "bdetr.h").read_text()
    assert "K16" in full and "K17" in full
    assert "-ffp-contract=off" in build.PER_FILE_FLAGS["detmetric.hip"] and "-ffp-contract=off" in build.PER_FILE_FLAGS["maskmetric.hip"]
    assert callable(kernels.det_match_coco) and callable(kernels.mask_match_coco)
    assert issubclass(evaluation.CocoEvaluator, evaluation.DetectionEvaluator) and issubclass(evaluation.CocoMaskEvaluator, evaluation.CocoEvaluator)
    import inspect
    assert inspect.signature(training.Model.evaluate).parameters["coco"].default is False
    assert inspect.signature(training.DetectionAP.__init__).parameters["coco"].default is False
    assert inspect.signature(pipeline.coco_records).parameters["with_eval_fields"].default is False
    import __graft_entry__
    __graft_entry__.build()
    h = _lib.lib()
    assert h.bdetr_abi_version() == 8 and hasattr(h, "bdetr_det_match_coco") and hasattr(h, "bdetr_mask_match_coco")
    assert hasattr(h, "bdetr_det_match") and hasattr(h, "bdetr_mask_match")


def test_pipeline_carries_eval_fields_only_when_asked():
    from boosted_detr_amd import pipeline
    coco = {"images": [{"id": 1, "width": 200, "height": 100, "file_name": "a.jpg"}, {"id": 2, "width": 50, "height": 50}],
            "categories": [{"id": 7, "name": "cat"}],
            "annotations": [{"image_id": 1, "category_id": 7, "bbox": [20, 10, 100, 50], "iscrowd": 1, "area": 4321.5},
                            {"image_id": 1, "category_id": 7, "bbox": [0, 0, 10, 20]}]}
    plain = pipeline.coco_records(coco)
    assert "iscrowd" not in plain[0] and set(pipeline.pad_annotations(plain, 3)) == {"category", "attribute", "bbox", "num_objects"}
    recs = pipeline.coco_records(coco, with_eval_fields=True)
    assert recs[0]["iscrowd"] == [1, 0] and recs[0]["area"] == [4321.5, 200.0] and recs[1]["iscrowd"] == []
    batch = pipeline.pad_annotations(recs, 3, with_eval_fields=True)
    assert batch["iscrowd"].tolist() == [[1, 0, 0], [0, 0, 0]] and batch["area"].tolist() == [[4321.5, 200.0, 0.0], [0.0, 0.0, 0.0]]
    assert batch["height"].tolist() == [100, 50] and batch["width"].tolist() == [200, 50] and batch["iscrowd"].dtype == np.int32
    assert np.array_equal(batch["bbox"], pipeline.pad_annotations(plain, 3)["bbox"])


# ---------------------------------------------------------------------------------------------------------------------
# 6. one precision / recall curve: the short form is the COCO form without ignore bits and without a rank cut
# ---------------------------------------------------------------------------------------------------------------------
SHORT_FORM = json.loads((ROOT / "tests" / "golden" / "short_form_ap.json").read_text())["cases"]


def unhex(v):
    return float("nan") if v is None else float.fromhex(v)


@pytest.mark.parametrize("name", sorted(CS.BOX_CASES))
def test_one_curve_serves_both_protocols(name):
    from boosted_detr_amd import evaluation
    c, images = CS.BOX_CASES[name], CS.reference(name)
    for b, im in enumerate(images):
        im.update(score=c["score"][b], label=c["label"][b])
    T, N = len(c["thresholds"]), c["score"].shape[1]
    gt_count = sum(im["gt_count"] for im in images)[0]
    short = [(im["score"][None].astype(np.float32), np.asarray(im["label"], np.int32)[None], R.pack_bits(im["keep"], im["tp"][0])[None],
              np.asarray(im["order"], np.int32)[None]) for im in images]
    full = [(s, l, im["class_rank"][None].astype(np.int32), t[None], np.zeros_like(t)[None], o) for (s, l, t, o), im in zip(short, images)]
    got = evaluation.DetectionEvaluator(c["C"], c["thresholds"], N).result_from(short, gt_count)
    want = SHORT_FORM[name]                                                      # what the short form's own loop gave before there was one
    for k in ("AP", "AP50", "AP75", "AR"):
        assert exactly(got[k], unhex(want[k])), (k, got[k], unhex(want[k]))
    assert np.array_equal(got["per_class_AP"], [unhex(v) for v in want["per_class_AP"]], equal_nan=True)
    assert got["num_detections"] == want["num_detections"] and np.array_equal(got["gt_count"], gt_count)
    # the function both call, class by class, against the arrays of accumulate_pair
    lineup = evaluation._Lineup(full, 1)
    precision, recall = evaluation.accumulate_pair(lineup, gt_count, T, 0, N)
    assert precision.shape == (T, 101, c["C"]) and (gt_count > 0).any()
    for cls in range(c["C"]):
        if gt_count[cls] == 0:
            assert (precision[:, :, cls] == -1).all() and (recall[:, cls] == -1).all()
            continue
        sel = lineup.labels == cls
        for ig in (None, lineup.ig[0][sel]):                                     # no ignore words, or all-zero ones
            p, r = evaluation.precision_recall(lineup.scores[sel], lineup.tp[0][sel], ig, int(gt_count[cls]), T)
            assert p.shape == (T, 101) and r.shape == (T,)
            assert np.array_equal(p, precision[:, :, cls]) and np.array_equal(r, recall[:, cls]), cls


# ---------------------------------------------------------------------------------------------------------------------
# 7. the one device-to-host copy: every kept tensor comes back with its shape, its host dtype and its bits
# ---------------------------------------------------------------------------------------------------------------------
def _filled_evaluators():
    """A DetectionEvaluator, a CocoEvaluator with two ranges and a PanopticEvaluator, two batches each of different shapes, with
    host tensors standing in for device tensors and values that a careless widening would change."""
    import torch
    from boosted_detr_amd import evaluation
    rng = np.random.default_rng(5)
    C, A = 5, 2
    det = evaluation.DetectionEvaluator(C)
    coco = evaluation.CocoEvaluator(C, area_ranges={"all": (0.0, 1e10), "small": (0.0, 1024.0)})
    pq = evaluation.PanopticEvaluator(C, stuff_classes=(4,))

    def i32(*shape, lo=2, hi=C):
        return torch.from_numpy(rng.integers(lo, hi, shape).astype(np.int32))

    def words(*shape):                                                           # uint16 patterns as the kernels store them: int16
        w = rng.integers(0, 1 << 10, shape).astype(np.uint16) | np.uint16(evaluation.KEEP_BIT)
        w.reshape(-1)[1] &= np.uint16(0x7FFF)                                    # one detection that was not kept
        return torch.from_numpy(w.view(np.int16).copy())

    for B, N, M in ((1, 3, 2), (2, 5, 4)):
        score = rng.random((B, N)).astype(np.float32)
        score[0, 0], score[0, 1] = -0.25, np.float32(np.nan)
        score.view(np.uint32)[0, 1] = 0x7FC00123                                 # a NaN with a payload
        score = torch.from_numpy(score)
        order = np.stack([rng.permutation(N) for _ in range(B)]).astype(np.int32)
        order[:, -1] = -1                                                        # a rank that holds no detection
        order = torch.from_numpy(order)
        label = i32(B, N)
        det._kept.append((score, label, words(B, N), order))
        coco._kept.append((score, label, i32(B, N, lo=0, hi=N), words(A, B, N), words(A, B, N), order))
        union = i32(B, M, lo=1, hi=1 << 30)
        pq._kept.append((i32(B, M, lo=-2, hi=N), i32(B, N, lo=-2, hi=M), (union.double() * 0.7).to(torch.int32), union, i32(B, M), i32(B, N)))
    det._gt_count = torch.tensor([0, 0, 3, 1, 2], dtype=torch.int32)
    coco._gt_count = torch.tensor([[0, 0, 3, 1, 2], [0, 0, 1, 0, 2]], dtype=torch.int32)
    return det, coco, pq


def _same_result(got, want):
    assert list(got) == list(want)
    for k, w in want.items():
        g = got[k]
        if isinstance(w, np.ndarray):
            assert isinstance(g, np.ndarray) and g.dtype == w.dtype and np.array_equal(g, w, equal_nan=True), k
        elif isinstance(w, list):
            assert len(g) == len(w) and all(exactly(x, y) for x, y in zip(g, w)), k
        else:
            assert type(g) is type(w) and (exactly(g, w) if isinstance(w, float) else g == w), k


def test_the_host_copy_returns_every_field_as_it_went_in(monkeypatch):
    import torch
    from boosted_detr_amd import evaluation
    det, coco, pq = _filled_evaluators()
    host16 = {torch.float32: np.float32, torch.int32: np.int32, torch.int16: np.uint16}

    def check_records(ev, records):
        assert len(records) == len(ev._kept) == 2
        for rec, kept in zip(records, ev._kept):
            assert len(rec) == len(kept)
            for k, (h, d) in enumerate(zip(rec, kept)):
                assert h.dtype == host16[d.dtype] and h.shape == tuple(d.shape), (k, h.dtype, h.shape)
                assert h.tobytes() == d.numpy().tobytes(), k                     # bit for bit, NaN payloads and bit 15 included

    for ev, shape in ((det, (5,)), (coco, (2, 5))):
        records, gt_count = ev._to_host()
        check_records(ev, records)
        assert gt_count.dtype == np.int64 and gt_count.shape == shape and np.array_equal(gt_count, ev._gt_count.numpy())
    records = pq._to_host()
    assert isinstance(records, list)
    check_records(pq, records)
    assert records[1][0].min() < 0 and det._to_host()[0][0][3].min() == -1 and (det._to_host()[0][0][2] & evaluation.KEEP_BIT).any()

    alone = [ev.result() for ev in (det, coco, pq)]
    assert alone[0]["num_images"] == alone[1]["num_images"] == alone[2]["num_images"] == 3 and alone[0]["num_detections"] > 0
    copies = []
    cat = torch.cat
    monkeypatch.setattr(torch, "cat", lambda *a, **k: copies.append(1) or cat(*a, **k))
    together = evaluation.results([det, coco, pq])
    assert len(copies) == 1                                                      # one torch.cat(...).cpu() for the three
    for got, want in zip(together, alone):
        _same_result(got, want)
    empty = evaluation.CocoEvaluator(5, area_ranges={"all": (0.0, 1e10), "small": (0.0, 1024.0)})
    for middle, fresh in ((empty, evaluation.CocoEvaluator(5, area_ranges={"all": (0.0, 1e10), "small": (0.0, 1024.0)}).result()),
                          (evaluation.PanopticEvaluator(5), evaluation.PanopticEvaluator(5).result()),
                          (evaluation.DetectionEvaluator(5), evaluation.DetectionEvaluator(5).result())):
        got = evaluation.results([det, middle, pq, coco])
        for g, w in zip(got, [alone[0], fresh, alone[2], alone[1]]):
            _same_result(g, w)
    assert empty._to_host()[0] == [] and empty._to_host()[1].shape == (2, 5) and evaluation.PanopticEvaluator(5)._to_host() == []
    assert [r for r in evaluation.results([evaluation.DetectionEvaluator(5)])][0]["num_detections"] == 0
