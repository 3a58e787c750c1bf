"""Host half of the panoptic-quality path (no GPU): the plain-loop reference (tests/_panoptic_ref.py) on hand-worked cases whose
PQ / SQ / RQ are written out in tests/_panoptic_cases.py, evaluation.PanopticEvaluator's host side (validation, empty result, the
things / stuff split, result() from injected integer tensors) and every refusal that comes before the library is touched.

panopticapi is not a dependency of this project; where it cannot be imported the comparison against its pq_compute_single_core
is not part of the suite (the hand-worked numbers below are the standard)."""
import numpy as np
import pytest
import torch

import _panoptic_cases as PC
import _panoptic_ref as P

G = 23


def reference_image(c):
    """A hand-worked case through the reference's exclusive ground truth, joint counts and matching."""
    excl, gt_ids, gt_pop = P.gt_exclusive(c["gt_masks"], c["gt_label"], c["num_objects"], PC.C)
    assert np.array_equal(excl, c["gt_masks"] & (np.arange(PC.M) < c["num_objects"])[:, None, None] & (c["gt_label"] >= 2)[:, None, None])
    pred_pop = np.asarray([(c["pred_ids"] == n).sum() for n in range(PC.N)], np.int64)
    inter = P.joint_counts(c["pred_ids"], gt_ids, PC.N, PC.M)
    out = P.match(inter, pred_pop, c["pred_label"], c["seg_of"], gt_pop, c["gt_label"], c["gt_crowd"], c["num_objects"], PC.C, c["min_area"])
    out.update(gt_label=c["gt_label"], pred_label=c["pred_label"], inter=inter, pred_pop=pred_pop, gt_pop=gt_pop)
    return out


def record_of(images):
    """Images of one shape as one batch, the way bdetr_panoptic_match leaves it: int32 [B,M] / [B,N] host arrays."""
    keys = ("gt_state", "pred_state", "match_inter", "match_union", "gt_label", "pred_label")
    return tuple(np.stack([np.asarray(im[k], np.int32) for im in images]) for k in keys)


@pytest.mark.parametrize("name", list(PC.CASES))
def test_reference_on_hand_worked_cases(name):
    c = PC.CASES[name]
    want = c["want"]
    im = reference_image(c)
    assert im["pred_state"].tolist() == want["pred_state"] and im["gt_state"].tolist() == want["gt_state"], (im["pred_state"], im["gt_state"])
    matched = [m for m, s in enumerate(want["gt_state"]) if s >= 0]
    assert all(im["match_inter"][m] > 0 and im["match_union"][m] > 0 for m in matched)
    assert all(im["match_inter"][m] == 0 and im["match_union"][m] == 0 for m in range(PC.M) if m not in matched)
    for k in ("match_inter", "match_union"):
        if k in want:
            assert im[k].tolist() == want[k], k
    r = P.pq([im], PC.C)
    assert (sum(r["tp"]), sum(r["fp"]), sum(r["fn"])) == (want["tp"], want["fp"], want["fn"])
    assert (r["PQ"], r["SQ"], r["RQ"]) == (want["PQ"], want["SQ"], want["RQ"]) and r["num_classes_scored"] == want["classes"]
    # the evaluator's host half on the same integers: the same numbers
    from boosted_detr_amd.evaluation import PanopticEvaluator
    got = PanopticEvaluator(PC.C, min_area=c["min_area"]).result_from([record_of([im])])
    assert (got["PQ"], got["SQ"], got["RQ"]) == (want["PQ"], want["SQ"], want["RQ"]) and got["num_classes_scored"] == want["classes"]
    assert (int(got["tp"].sum()), int(got["fp"].sum()), int(got["fn"].sum())) == (want["tp"], want["fp"], want["fn"]) and got["num_images"] == 1


def test_reference_rules():
    # select: a score equal to the threshold and a NaN are dropped; stuff merges into the lowest KEPT query of the class
    score = np.asarray([0.5, 0.9, 0.85, 0.95, np.nan, 0.99, 0.9], np.float32)
    label = np.asarray([3, 3, 3, 2, 2, 3, 2])
    stuff = np.asarray([0, 0, 0, 1, 0, 0], np.uint8)
    assert P.select(score, label, stuff, 0.85).tolist() == [-1, 1, -1, 3, -1, 1, 6]
    assert P.select(score, label, None, 0.85).tolist() == [-1, 1, -1, 3, -1, 5, 6]
    assert P.select(score, label, stuff, 0.0).tolist() == [0, 0, 0, 3, -1, 0, 6]
    # merge: equal logits -> the lower query; nothing positive -> void; NaN never wins
    L = np.zeros((4, 2, 2), np.float32)
    L[0], L[1], L[2], L[3] = 1.0, 1.0, -1.0, np.nan
    assert (P.merge(L, [0, 1, 2, 3], 3, 5) == 0).all()
    assert (P.merge(L, [-1, 1, 2, 3], 3, 5) == 1).all()
    assert (P.merge(L, [-1, -1, 2, 3], 3, 5) == -1).all()
    assert (P.merge(L, [-1, 0, -1, -1], 3, 5) == 0).all()          # the id is seg_of of the winner, not the winner
    # the exclusive ground truth: the lowest segment row wins; label 0, rows past num_objects and hidden rows are no segments
    masks = np.zeros((5, 2, 4), bool)
    masks[0, :, :2], masks[1, :, 1:3], masks[2], masks[3, 0, 0], masks[4] = True, True, True, True, True
    excl, gt_ids, gt_pop = P.gt_exclusive(masks, [2, 3, 0, 4, 2], 4, 5)
    assert gt_ids.tolist() == [[0, 0, 1, -1], [0, 0, 1, -1]] and gt_pop.tolist() == [4, 2, 0, 0, 0] and not excl[2:].any()
    assert P.joint_counts(np.asarray([[0, 0, 1, 1], [-1, 2, 2, 2]]), gt_ids, 3, 5)[:, :2].tolist() == [[2, 0], [0, 1], [1, 1]]


def test_result_from_injected_tensors_and_the_split():
    from boosted_detr_amd.evaluation import PanopticEvaluator, accumulate_pq
    images = [reference_image(c) for c in PC.CASES.values()]
    # two batches of different sizes, in order
    records = [record_of(images[:3]), record_of(images[3:])]
    for stuff in ((), (3,), (2, 3, 4, 5)):
        want = P.pq(images, PC.C, stuff)
        got = PanopticEvaluator(PC.C, stuff_classes=stuff).result_from(records)
        assert got["tp"].tolist() == want["tp"] and got["fp"].tolist() == want["fp"] and got["fn"].tolist() == want["fn"]
        for suffix in ("", "_th", "_st"):
            for k in ("PQ", "SQ", "RQ"):
                assert abs(got[k + suffix] - want[k + suffix]) <= 1e-12, (stuff, k + suffix, got[k + suffix], want[k + suffix])
            assert got["num_classes_scored" + suffix] == want["num_classes_scored" + suffix]
        for c in range(PC.C):
            if c in want["per_class"]:
                assert all(abs(got["per_class_" + k][c] - want["per_class"][c][i]) <= 1e-12 for i, k in enumerate(("PQ", "SQ", "RQ")))
            else:
                assert all(np.isnan(got["per_class_" + k][c]) for k in ("PQ", "SQ", "RQ"))
        assert got["num_images"] == len(images)
    # hand-worked: class 2 has tp 2 (IoU 1 and 2/3), fp 3, fn 3; class 3 has tp 2 (IoU 1 twice), fn 2
    all_ = PanopticEvaluator(PC.C).result_from(records)
    assert (all_["tp"].tolist(), all_["fp"].tolist(), all_["fn"].tolist()) == ([0, 0, 2, 2, 0, 0], [0, 0, 3, 0, 0, 0], [0, 0, 3, 2, 0, 0])
    assert abs(all_["per_class_PQ"][2] - (1.0 + 2.0 / 3.0) / 5.0) <= 1e-15 and abs(all_["per_class_PQ"][3] - 2.0 / 3.0) <= 1e-15
    split = PanopticEvaluator(PC.C, stuff_classes=(3,)).result_from(records)
    assert split["PQ_th"] == all_["per_class_PQ"][2] and split["PQ_st"] == all_["per_class_PQ"][3] and split["num_classes_scored_st"] == 1
    none = PanopticEvaluator(PC.C, stuff_classes=(5,)).result_from(records)
    assert (none["PQ_st"], none["SQ_st"], none["RQ_st"], none["num_classes_scored_st"]) == (0.0, 0.0, 0.0, 0) and none["PQ_th"] == all_["PQ"]
    assert accumulate_pq([], PC.C)["num_images"] == 0


def test_empty_result_and_reset():
    from boosted_detr_amd.evaluation import PanopticEvaluator
    ev = PanopticEvaluator(7, stuff_classes=(4,))
    res = ev.result()
    assert all(res[k + s] == 0.0 for k in ("PQ", "SQ", "RQ") for s in ("", "_th", "_st"))
    assert res["num_classes_scored"] == 0 and res["num_images"] == 0 and res["tp"].shape == (7,) and not res["tp"].any()
    assert np.isnan(res["per_class_PQ"]).all()
    assert set(res) >= {"PQ", "SQ", "RQ", "PQ_th", "SQ_th", "RQ_th", "PQ_st", "SQ_st", "RQ_st", "per_class_PQ", "per_class_SQ", "per_class_RQ",
                        "tp", "fp", "fn", "num_classes_scored", "num_images"}
    ev._kept.append("x")
    ev.reset()
    assert ev._kept == [] and ev.last is None
    assert (ev.score_threshold, ev.min_area, ev.stuff_classes) == (0.85, 5, (4,))


def test_constructor_validation():
    from boosted_detr_amd.evaluation import PanopticEvaluator
    assert PanopticEvaluator(7, stuff_classes=[6, 2, np.int32(2)]).stuff_classes == (2, 6)
    for bad in ((1,), (7,), (-1,), (2.5,), ("3",), (True,), (0,)):
        with pytest.raises(ValueError, match="stuff_classes"):
            PanopticEvaluator(7, stuff_classes=bad)
    for kw, match in ((dict(score_threshold=1.0), "score_threshold"), (dict(score_threshold=-0.1), "score_threshold"),
                      (dict(score_threshold=float("nan")), "score_threshold"), (dict(min_area=-1), "min_area"), (dict(min_area=2.5), "min_area"),
                      (dict(max_mask_bytes=0), "positive")):
        with pytest.raises(ValueError, match=match):
            PanopticEvaluator(7, **kw)
    with pytest.raises(ValueError, match="at least 3"):
        PanopticEvaluator(2)


# ---------------------------------------------------------------- refusals
def _records():
    return [{"height": 20, "width": 30, "bbox": [[0.1, 0.1, 0.5, 0.5], [0.2, 0.2, 0.3, 0.3]], "category": [["a"], ["b"]], "attribute": [["x"], ["y"]],
             "iscrowd": [0, 1], "area": [50.0, 20.0], "segmentation": [[[3, 3, 20, 3, 20, 15, 3, 15]], {"size": [20, 30], "counts": [40, 30, 530]}]},
            {"height": 12, "width": 70, "bbox": [[0.0, 0.0, 1.0, 1.0]], "category": [["a"]], "attribute": [["x"]], "iscrowd": [0], "area": [9.0],
             "segmentation": [None]}]


@pytest.fixture()
def no_library(monkeypatch):
    """Any touch of the library, or of a device, fails the test."""
    from boosted_detr_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched before the refusal")

    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(torch.Tensor, "cuda", boom)


def test_evaluator_refusals_come_before_the_library(no_library):
    from boosted_detr_amd import pipeline
    from boosted_detr_amd.evaluation import CocoImageMaskEvaluator, PanopticEvaluator, host_image_hw
    batch = pipeline.pad_annotations(_records(), with_eval_fields=True, with_masks=True)
    B, M, N, Cc = 2, 2, 6, 5
    hw = host_image_hw(batch["height"], batch["width"])
    ev = PanopticEvaluator(Cc)
    assert ev.max_mask_bytes == CocoImageMaskEvaluator.DEFAULT_MAX_MASK_BYTES == 1 << 30
    assert ev.check_batch(batch["segments"], hw, N)[1:] == (20, 2)
    cat_pred, logits = torch.zeros(B, N, Cc), torch.zeros(B, N, G, G)
    cat_ids, num_objects = torch.zeros(B, M, dtype=torch.int32), torch.tensor([2, 1], dtype=torch.int32)

    def bad(match, segments=batch["segments"], image_hw=hw, evaluator=ev, **kw):
        with pytest.raises(ValueError, match=match) as e:
            evaluator.update(kw.get("cat_pred", cat_pred), kw.get("logits", logits), cat_ids, segments, num_objects, image_hw)
        assert evaluator._kept == [] and evaluator.last is None
        return str(e.value)

    bad("with_masks=True", segments=None)
    bad("with_masks=True", segments={"masks": np.zeros((B, M, G, G), np.float32)})
    bad("integers \\[B=2,2\\]", image_hw=hw[:1])
    bad("integers \\[B=2,2\\]", image_hw=hw.astype(np.float32))
    wrong = dict(batch["segments"], hw=batch["segments"]["hw"].copy())
    wrong["hw"][0, 1] = (30, 20)
    said = bad("object 1 of image 0 was annotated on a \\(30, 20\\) image", segments=wrong)
    with pytest.raises(ValueError) as e:             # the same refusal, word for word, as the image-resolution mask evaluator's
        CocoImageMaskEvaluator(Cc).check_batch(wrong, hw, N)
    assert str(e.value) == said
    need = 8 * 20 * 2 * B * (N + M)
    said = bad(f"need {need} bytes", evaluator=PanopticEvaluator(Cc, max_mask_bytes=need - 1))
    with pytest.raises(ValueError) as e:
        CocoImageMaskEvaluator(Cc, max_mask_bytes=need - 1).check_batch(batch["segments"], hw, N)
    assert str(e.value) == said
    assert PanopticEvaluator(Cc, max_mask_bytes=need).check_batch(batch["segments"], hw, N)[1:] == (20, 2)
    bad("4096", image_hw=np.asarray([[20, 30], [12, 4097]], np.int32))
    bad("classes", cat_pred=torch.zeros(B, N, Cc + 1))
    bad("square grid", logits=torch.zeros(B, N, 5, 4))

    class FakeDeviceTensor:
        is_cuda = True

    bad("not a device tensor", image_hw=FakeDeviceTensor())


def test_model_refusals_come_before_the_library(no_library):
    from boosted_detr_amd import pipeline
    from boosted_detr_amd.evaluation import CocoImageMaskEvaluator, PanopticEvaluator
    from boosted_detr_amd.training import Model, PanopticQuality

    class Headed(Model):                             # a model with a mask head, as far as evaluate_panoptic() asks before the first batch
        num_categories, num_object_preds, _panoptic_inputs = 5, 6, None

        def _require_panoptic_head(self):
            pass

    model = Headed.__new__(Headed)
    batch = pipeline.pad_annotations(_records(), with_eval_fields=True, with_masks=True)

    def bad(match, b, **kw):
        with pytest.raises(ValueError, match=match):
            model.evaluate_panoptic([b], **kw)

    bad("with_masks=True", {k: v for k, v in batch.items() if k != "segments"})
    bad("'height' and 'width'", {k: v for k, v in batch.items() if k != "height"})
    bad("object 0 of image 0 was annotated on a \\(20, 30\\) image", dict(batch, height=np.asarray([21, 12], np.int32)))
    bad("max_mask_bytes is 100", batch, evaluator=PanopticEvaluator(5, max_mask_bytes=100))
    bad("PanopticEvaluator", batch, evaluator=CocoImageMaskEvaluator(5))
    bad("stuff_classes", batch, stuff_classes=(5,))
    bad("score_threshold", batch, score_threshold=1.0)
    with pytest.raises(ValueError, match="stuff_classes"):
        model.panoptic_segmentation({"image": None, "height": [20, 12], "width": [30, 70]}, stuff_classes=(1,))
    with pytest.raises(ValueError, match="'height' and 'width'"):
        model.panoptic_segmentation({"image": None})
    # a model without a mask head refuses both before it looks at anything else
    plain = Model.__new__(Model)
    with pytest.raises(RuntimeError, match="no mask head"):
        plain.evaluate_panoptic([batch])
    with pytest.raises(RuntimeError, match="no mask head"):
        plain.panoptic_segmentation(batch)
    cb = PanopticQuality([batch], every=2, steps=3, score_threshold=0.5, min_area=2, stuff_classes=[3])
    assert (cb.every, cb.steps, cb.score_threshold, cb.min_area, cb.stuff_classes) == (2, 3, 0.5, 2, (3,))


def test_wrappers_check_dtypes_and_shapes_before_the_library(no_library):
    from boosted_detr_amd import _lib
    from boosted_detr_amd import kernels as K
    f, i = torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(_lib.BdetrError, match="label must be a torch.int32"):
        K.panoptic_select(f, f, 0.5, 5)
    with pytest.raises(_lib.BdetrError, match="shapes disagree"):
        K.panoptic_select(f, i[:1], 0.5, 5)
    with pytest.raises(ValueError, match="threshold"):
        K.panoptic_select(f, i, 1.0, 5)
    with pytest.raises(_lib.BdetrError, match="is_stuff must be a torch.uint8"):
        K.panoptic_select(f, i, 0.5, 5, is_stuff=torch.zeros(5))
    with pytest.raises(_lib.BdetrError, match="seg_of must be a torch.int32"):
        K.panoptic_merge(torch.zeros(2, 3, 4, 4), f, torch.zeros(2, 2, dtype=torch.int32), 8, 1)
    with pytest.raises(_lib.BdetrError, match=r"logits must be \[B,N,G,G\]"):
        K.panoptic_merge(torch.zeros(2, 3, 4, 5), i, torch.zeros(2, 2, dtype=torch.int32), 8, 1)
    with pytest.raises(ValueError, match="Wm"):
        K.panoptic_merge(torch.zeros(2, 3, 4, 4), i, torch.zeros(2, 2, dtype=torch.int32), 8, 65)
    with pytest.raises(_lib.BdetrError, match="gt_bits must be a torch.int64"):
        K.panoptic_gt_exclusive(torch.zeros(2, 3, 8, 1), i, torch.zeros(2, dtype=torch.int32), 5)
    with pytest.raises(_lib.BdetrError, match="shapes disagree"):
        K.panoptic_gt_exclusive(torch.zeros(2, 3, 8, 1, dtype=torch.int64), i[:, :2], torch.zeros(2, dtype=torch.int32), 5)
    inter = torch.zeros(2, 3, 4, dtype=torch.int32)
    g = torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(_lib.BdetrError, match="shapes disagree"):
        K.panoptic_match(inter, i, i, i, g, i, None, torch.zeros(2, dtype=torch.int32), 5, 5)
    with pytest.raises(_lib.BdetrError, match="gt_crowd must be a torch.uint8"):
        K.panoptic_match(inter, i, i, i, g, g, g, torch.zeros(2, dtype=torch.int32), 5, 5)
    with pytest.raises(ValueError, match="min_area"):
        K.panoptic_match(inter, i, i, i, g, g, None, torch.zeros(2, dtype=torch.int32), 5, -1)


# ---------------------------------------------------------------- declarations and limits
NEW = ("bdetr_panoptic_select", "bdetr_panoptic_merge", "bdetr_panoptic_gt_exclusive", "bdetr_panoptic_match")


def test_new_symbols_are_declared_and_refuse_bad_sizes_on_the_host():
    import ctypes as C
    import re
    from pathlib import Path
    from boosted_detr_amd import _lib, build, evaluation, kernels, training
    raw = (Path(__file__).resolve().parent.parent / "include" / "bdetr.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"#define\s+BDETR_ABI_VERSION\s+8\b", raw)
    for k in ("K23", "K24", "K25", "K26", "PostProcessPanoptic", "panopticapi"):
        assert re.search(rf"\b{k}\b", raw), k
    for name in NEW:
        decl = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)", header)
        assert decl, f"{name} is not declared in include/bdetr.h"
        kinds = [C.c_void_p if "*" in a else C.c_float if a.strip().startswith("float") else C.c_int for a in decl.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == kinds, name
    assert "panopticmerge.hip" in build.SOURCES and "-ffp-contract=off" in build.PER_FILE_FLAGS["panopticmerge.hip"]
    for fn in ("panoptic_select", "panoptic_merge", "panoptic_gt_exclusive", "panoptic_match"):
        assert callable(getattr(kernels, fn)), fn
    assert callable(training.Model.evaluate_panoptic) and callable(training.Model.panoptic_segmentation)
    assert issubclass(training.PanopticQuality, training.Callback) and training.Model.IOU_TYPES == ("bbox", "segm")
    assert not issubclass(evaluation.PanopticEvaluator, evaluation.DetectionEvaluator)
    import __graft_entry__
    __graft_entry__.build()
    h = _lib.lib()
    assert h.bdetr_abi_version() == 8 and all(hasattr(h, name) for name in NEW)
    # the entries refuse bad sizes without a launch (no GPU is touched)
    err = h.bdetr_last_error
    assert h.bdetr_panoptic_select(1, 1, None, 1, 1025, 5, 0.5, 1, None) == -1 and b"N in [1, 1024]" in err()
    assert h.bdetr_panoptic_select(1, 1, None, 1, 9, 5, 1.0, 1, None) == -1 and b"threshold must be in [0, 1)" in err()
    assert h.bdetr_panoptic_select(1, 1, None, 1, 9, 5, float("nan"), 1, None) == -1 and b"threshold" in err()
    assert h.bdetr_panoptic_select(1, None, None, 1, 9, 5, 0.5, 1, None) == -1 and b"null pointer" in err()
    assert h.bdetr_panoptic_merge(1, 1, 1, 1, 9, 33, 8, 1, 16, None, 1, None) == -1 and b"G in [1, 32]" in err()
    assert h.bdetr_panoptic_merge(1, 1, 1, 1, 9, 23, 8, 65, 16, None, 1, None) == -1 and b"Wm in [1, 64]" in err()
    assert h.bdetr_panoptic_merge(1, 1, 1, 1, 1025, 23, 8, 1, 16, None, 1, None) == -1 and b"N in [1, 1024]" in err()
    assert h.bdetr_panoptic_merge(1, 1, 1, 1, 9, 23, 8, 1, 18, None, 1, None) == -1 and b"16-byte aligned" in err()
    assert h.bdetr_panoptic_merge(1, 1, 1, 1, 9, 23, 8, 1, None, None, 1, None) == -1 and b"null pointer" in err()
    assert h.bdetr_panoptic_gt_exclusive(1, 1, 1, 1, 1025, 5, 8, 1, 1, None) == -1 and b"M in [1, 1024]" in err()
    assert h.bdetr_panoptic_gt_exclusive(1, 1, 1, 1, 6, 2, 8, 1, 1, None) == -1 and b"C in [3, 65536]" in err()
    assert h.bdetr_panoptic_gt_exclusive(1, 1, 1, 1, 6, 5, 4097, 1, 1, None) == -1 and b"Hm in [1, 4096]" in err()
    assert h.bdetr_panoptic_match(*[1] * 6, None, 1, 1, 9, 6, 5, -1, 1, 1, 1, 1, None) == -1 and b"min_area >= 0" in err()
    assert h.bdetr_panoptic_match(*[1] * 6, None, 1, 1, 9, 1025, 5, 5, 1, 1, 1, 1, None) == -1 and b"M in [1, 1024]" in err()
    assert h.bdetr_panoptic_match(*[1] * 6, None, 1, 1, 9, 6, 5, 5, 1, 1, None, 1, None) == -1 and b"null pointer" in err()


def test_models_without_a_mask_head_refuse():
    from boosted_detr_amd.boosted_model import BoostedDETR
    from boosted_detr_amd.model import DETR
    boosted = object.__new__(BoostedDETR)
    plain = object.__new__(DETR)
    plain.__dict__["PanopticAttention"] = None               # what DETR() without with_panoptic_head leaves
    for model, match in ((boosted, "BoostedDETR has no mask head"), (plain, "with_panoptic_head=True")):
        with pytest.raises(RuntimeError, match=match):
            model.evaluate_panoptic([])
        with pytest.raises(RuntimeError, match=match):
            model.panoptic_segmentation({})
