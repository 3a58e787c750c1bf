"""CPU half of the image-resolution mask path (K19-K22): the upsample rule of include/bdetr.h against torch's bilinear interpolate,
its identity at grid size, the declarations, and every refusal - raised before the library is touched."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _coco_ref as R
import _mask_image_ref as MI

ROOT = Path(__file__).resolve().parent.parent
G = 23
NEW = ("bdetr_mask_upsample_bits", "bdetr_mask_source_bits", "bdetr_mask_inter", "bdetr_mask_match_coco_inter")


# ---------------------------------------------------------------- the rule
def test_rule_agrees_with_torch_bilinear_away_from_zero():
    rng = np.random.default_rng(5)
    total = excluded = 0
    for (h, w) in [(5, 7), (23, 23), (37, 61), (64, 64), (65, 130)]:
        L = (3.0 * rng.standard_normal((4, G, G))).astype(np.float32)
        want = torch.nn.functional.interpolate(torch.from_numpy(L)[None], size=(h, w), mode="bilinear", align_corners=False)[0].numpy()
        for k in range(4):
            v = MI.upsample(L[k], h, w)
            assert v.shape == (h, w) and v.dtype == np.float64
            far = np.abs(v) >= 1e-4
            assert np.array_equal((v > 0)[far], (want[k] > 0)[far]), (h, w, k)
            assert np.array_equal(MI.upsample_mask(L[k], h, w), v > 0)
            total += v.size
            excluded += int((~far).sum())
    assert excluded <= 1e-3 * total, (excluded, total)


def test_rule_is_the_identity_at_grid_size():
    rng = np.random.default_rng(6)
    L = (3.0 * rng.standard_normal((G, G))).astype(np.float32)
    L[3, 4], L[5, 5] = 0.0, -0.0
    v = MI.upsample(L, G, G)
    assert np.array_equal(v, L.astype(np.float64))
    assert np.array_equal(MI.upsample_mask(L, G, G), R.binarize(L, 0.0))
    ia, ib, t = MI.axis_rule(G, G)
    assert np.array_equal(ia, np.arange(G)) and (t == 0).all() and ib.max() == G - 1
    ia, ib, t = MI.axis_rule(130, G)                 # the first pixels lie left of the first cell's centre: num < 0, i0 = -1
    assert ia[0] == 0 and ib[0] == 0 and ia.max() == G - 1 and ib.max() == G - 1 and (t >= 0).all() and (t < 1).all()


def test_pack_layout_round_trip():
    rng = np.random.default_rng(7)
    m = rng.random((37, 130)) < 0.4
    bits = MI.pack(m, 40, 3)
    assert bits.shape == (40, 3) and bits.dtype == np.uint64
    assert np.array_equal(MI.unpack(bits, 37, 130), m) and int(MI.popcount(bits.reshape(1, -1))[0]) == int(m.sum())
    assert (bits[37:] == 0).all() and (bits[:, 2] >> np.uint64(2) == 0).all()          # rows past h and bits past w = 130 are zero
    assert bool((bits[5, 1] >> np.uint64(7)) & np.uint64(1)) == bool(m[5, 71])        # pixel (x = 71, y = 5)
    other = rng.random((37, 130)) < 0.4
    got = MI.inter(bits[None, None], MI.pack(other, 40, 3)[None, None], [1])
    assert got.shape == (1, 1, 1) and got[0, 0, 0] == int((m & other).sum())


# ---------------------------------------------------------------- declarations
def test_new_symbols_are_declared():
    from boosted_detr_amd import _lib, build, evaluation, kernels, training
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "bdetr.h").read_text(), flags=re.S)
    raw = (ROOT / "include" / "bdetr.h").read_text()
    assert re.search(r"#define\s+BDETR_ABI_VERSION\s+8\b", raw)
    for k in ("K19", "K20", "K21", "K22"):
        assert re.search(rf"\b{k}\b", raw), k
    for name in NEW:
        decl = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)", header)
        assert decl, f"{name} is not declared in include/bdetr.h"
        kinds = []
        for arg in decl.group(1).split(","):
            arg = arg.strip()
            kinds.append(C.c_void_p if "*" in arg else C.c_int64 if arg.startswith("int64_t") else C.c_int)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == kinds, name
    assert "maskimage.hip" in build.SOURCES and "-ffp-contract=off" in build.PER_FILE_FLAGS["maskimage.hip"]
    for fn in ("mask_upsample_bits", "mask_source_bits", "mask_inter", "mask_match_coco_inter"):
        assert callable(getattr(kernels, fn)), fn
    assert issubclass(evaluation.CocoImageMaskEvaluator, evaluation.CocoEvaluator)
    assert not issubclass(evaluation.CocoImageMaskEvaluator, evaluation.CocoMaskEvaluator)
    assert training.Model.MASK_RESOLUTIONS == ("grid", "image")
    import __graft_entry__
    __graft_entry__.build()
    h = _lib.lib()
    assert h.bdetr_abi_version() == 8 and all(hasattr(h, name) for name in NEW)
    # the entries refuse bad sizes without a launch (no GPU is touched)
    assert h.bdetr_mask_upsample_bits(1, 1, 1, 1, 33, 8, 1, 1, 1, None) == -1 and b"G in [1, 32]" in h.bdetr_last_error()
    assert h.bdetr_mask_upsample_bits(1, 1, 1, 1, 23, 8, 65, 1, 1, None) == -1 and b"Wm in [1, 64]" in h.bdetr_last_error()
    assert h.bdetr_mask_source_bits(None, 0, 1, 1, 1, 1, 1, 4097, 1, 1, 1, None) == -1 and b"Hm in [1, 4096]" in h.bdetr_last_error()
    assert h.bdetr_mask_source_bits(None, 0, None, 1, 1, 1, 1, 8, 1, 1, 1, None) == -1 and b"null pointer" in h.bdetr_last_error()
    assert h.bdetr_mask_inter(1, 1, 1, 1, 1025, 1, 8, 1, 1, None) == -1 and b"N in [1, 1024]" in h.bdetr_last_error()
    thr = (C.c_double * 1)(0.5)
    ptrs = [1] * 12 + [C.addressof(thr)]
    assert h.bdetr_mask_match_coco_inter(*ptrs, 1, 4, 4, 5, 1, 5, 100, 1, 1, 1, 1, 1, 1, None) == -1 and b"A in [1, 4]" in h.bdetr_last_error()
    assert h.bdetr_mask_match_coco_inter(*([1] * 2 + [None] + [1] * 9 + [C.addressof(thr)]), 1, 4, 4, 5, 1, 1, 100, 1, 1, 1, 1, 1, 1, None) == -1
    assert b"null pointer" in h.bdetr_last_error()


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
    from boosted_detr_amd.evaluation import CocoImageMaskEvaluator, host_image_hw
    batch = pipeline.pad_annotations(_records(), with_eval_fields=True, with_masks=True)
    B, M, N, Cc = 2, 2, 6, 5
    hw = host_image_hw(batch["height"], batch["width"])
    assert hw.dtype == np.int32 and hw.tolist() == [[20, 30], [12, 70]]
    ev = CocoImageMaskEvaluator(Cc)
    assert ev.max_mask_bytes == CocoImageMaskEvaluator.DEFAULT_MAX_MASK_BYTES == 1 << 30
    assert ev.check_batch(batch["segments"], hw, N)[1:] == (20, 2)
    cat_pred, logits = torch.zeros(B, N, Cc), torch.zeros(B, N, G, G)
    cat_ids, num_objects = torch.zeros(B, M, dtype=torch.int32), torch.tensor([2, 1], dtype=torch.int32)

    def bad(match, segments=batch["segments"], image_hw=hw, evaluator=ev, **kw):
        with pytest.raises(ValueError, match=match):
            evaluator.update(kw.get("cat_pred", cat_pred), logits, cat_ids, segments, num_objects, image_hw)
        assert evaluator._kept == [] and evaluator._gt_count is None

    bad("with_masks=True", segments=None)
    bad("with_masks=True", segments={"masks": np.zeros((B, M, G, G), np.float32)})          # dense masks are grid data
    bad("integers \\[B=2,2\\]", image_hw=hw[:1])
    bad("integers \\[B=2,2\\]", image_hw=hw.astype(np.float32))
    wrong = dict(batch["segments"], hw=batch["segments"]["hw"].copy())
    wrong["hw"][0, 1] = (30, 20)
    bad("object 1 of image 0 was annotated on a \\(30, 20\\) image", segments=wrong)
    unused = dict(batch["segments"], hw=batch["segments"]["hw"].copy())
    unused["hw"][1, 0] = (99, 99)                    # kind 0: not a segmented object, its hw means nothing
    assert ev.check_batch(unused, hw, N)[1:] == (20, 2)
    need = 8 * 20 * 2 * B * (N + M)
    bad(f"need {need} bytes", evaluator=CocoImageMaskEvaluator(Cc, max_mask_bytes=need - 1))
    assert CocoImageMaskEvaluator(Cc, max_mask_bytes=need).check_batch(batch["segments"], hw, N)[1:] == (20, 2)
    bad("4096", image_hw=np.asarray([[20, 30], [12, 4097]], np.int32))
    bad("classes", cat_pred=torch.zeros(B, N, Cc + 1))
    with pytest.raises(ValueError, match="positive"):
        CocoImageMaskEvaluator(Cc, max_mask_bytes=0)

    class FakeDeviceTensor:                          # what a device tensor answers, without a device
        is_cuda = True

    for name, kw in (("height", dict(height=FakeDeviceTensor(), width=batch["width"])), ("width", dict(height=batch["height"], width=FakeDeviceTensor()))):
        with pytest.raises(ValueError, match=f"'{name}' as a host array"):
            host_image_hw(**kw)
    bad("not a device tensor", image_hw=FakeDeviceTensor())
    with pytest.raises(ValueError, match="'height' and 'width'"):
        host_image_hw(None, batch["width"])
    assert host_image_hw(torch.tensor([20, 12]), [30, 70]).tolist() == hw.tolist()          # host tensors and sequences are fine


def test_model_refusals_come_before_the_library(no_library):
    from boosted_detr_amd import pipeline
    from boosted_detr_amd.evaluation import CocoImageMaskEvaluator, CocoMaskEvaluator
    from boosted_detr_amd.training import DetectionAP, Model

    class Headed(Model):                             # a model with a mask head, as far as evaluate() asks before the first batch
        num_categories, num_object_preds, _panoptic_inputs = 5, 6, None

        def _require_panoptic_head(self):
            pass

    model = Headed.__new__(Headed)
    batch = pipeline.pad_annotations(_records(), with_eval_fields=True, with_masks=True)
    both = ("bbox", "segm")
    with pytest.raises(ValueError, match="needs coco=True"):
        model.evaluate([batch], iou_types=both, mask_resolution="image")
    with pytest.raises(ValueError, match="needs coco=True"):
        DetectionAP([batch], iou_types=both, mask_resolution="image")
    with pytest.raises(ValueError, match="must be one of"):
        model.evaluate([batch], coco=True, mask_resolution="pixel")
    assert DetectionAP([batch], iou_types=both, coco=True, mask_resolution="image").mask_resolution == "image"
    assert DetectionAP([batch]).mask_resolution == "grid"
    with pytest.raises(ValueError, match="CocoImageMaskEvaluator"):
        model.evaluate([batch], coco=True, iou_types="segm", mask_resolution="image", mask_evaluator=CocoMaskEvaluator(5))

    def bad(match, b, **kw):
        with pytest.raises(ValueError, match=match):
            model.evaluate([b], coco=True, iou_types="segm", mask_resolution="image", **kw)

    bad("with_masks=True", {k: v for k, v in batch.items() if k != "segments"})
    bad("with_masks=True", dict({k: v for k, v in batch.items() if k != "segments"}, masks=np.zeros((2, 2, G, G), np.float32)))
    bad("'height' and 'width'", {k: v for k, v in batch.items() if k != "height"})
    bad("'height' and 'width'", {k: v for k, v in batch.items() if k != "width"})

    class FakeDeviceTensor:
        is_cuda = True

    bad("'width' as a host array", dict(batch, width=FakeDeviceTensor()))
    wrong = dict(batch, height=np.asarray([21, 12], np.int32))
    bad("object 0 of image 0 was annotated on a \\(20, 30\\) image", wrong)
    bad("max_mask_bytes is 100", batch, mask_evaluator=CocoImageMaskEvaluator(5, max_mask_bytes=100))
    with pytest.raises(ValueError, match="'height' and 'width'"):
        Model.segmentations(model, {"image": None}, resolution="image")
    with pytest.raises(ValueError, match="must be one of"):
        Model.segmentations(model, {"image": None}, resolution="pixel")


def test_detection_ap_asks_evaluate_for_what_its_arguments_say():
    """The callback's one call of Model.evaluate, with evaluate's defaults filled in, per way of building it; and the logs it leaves."""
    import inspect
    from boosted_detr_amd.training import DetectionAP, Model
    data, box_ev, mask_ev, both = [object()], object(), object(), ("bbox", "segm")
    four = ("AP", "AP50", "AP75", "AR")
    summary = four[:3] + ("AP_small", "AP_medium", "AP_large", "AR_1", "AR_10", "AR_100", "AR_small", "AR_medium", "AR_large") + four[3:]

    class Stub:
        def evaluate(self, *args, **kw):
            bound = inspect.signature(Model.evaluate).bind(self, *args, **kw)
            bound.apply_defaults()
            self.asked = {k: v for k, v in bound.arguments.items() if k != "self"}
            keys = summary if self.asked["coco"] else four
            res = {}
            for p, t in (("", "bbox"), ("mask_", "segm")):
                if t in self.asked["iou_types"]:
                    res.update({p + k: len(res) + 0.5 for k in keys})
                    res.update({f"per_class_{p}AP": np.zeros(3), p + "stats": [0.0], "num_images": 2})
            return res

    def run(keys, **kw):
        cb, model, logs = DetectionAP(data, steps=3, evaluator=box_ev, **kw), Stub(), {"loss": 1.0}
        cb.set_model(model)
        cb.on_epoch_end(0, logs)
        assert list(logs) == ["loss"] + ["val_" + k for k in keys] and cb.history == [{"epoch": 0, **{k: v for k, v in logs.items() if k != "loss"}}]
        assert all(type(logs[k]) is float for k in logs)
        return model.asked

    base = dict(x=data, steps=3, evaluator=box_ev, return_dict=True, verbose=0, iou_types=("bbox",), mask_evaluator=None, coco=False,
                mask_resolution="grid")
    assert run(four) == base
    assert run(four, mask_evaluator=mask_ev) == base                                         # without "segm" the short form never passed it on
    assert run(four + tuple("mask_" + k for k in four), iou_types=both, mask_evaluator=mask_ev) == dict(base, iou_types=both, mask_evaluator=mask_ev)
    assert run(tuple("mask_" + k for k in four), iou_types="segm") == dict(base, iou_types=("segm",))
    assert run(summary, coco=True, mask_evaluator=mask_ev) == dict(base, coco=True, mask_evaluator=mask_ev)
    assert run(summary + tuple("mask_" + k for k in summary), coco=True, iou_types=both, mask_resolution="image") == \
        dict(base, coco=True, iou_types=both, mask_resolution="image")
    cb = DetectionAP(data, every=2)
    cb.set_model(Stub())
    cb.on_epoch_end(0, {})
    assert cb.history == [] and not hasattr(cb.model, "asked")
    cb.on_epoch_end(1, None)
    assert [h["epoch"] for h in cb.history] == [1]
