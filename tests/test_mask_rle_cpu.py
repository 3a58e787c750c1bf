"""Host half of the COCO result-file export (K27 / K28, csrc/maskrle.hip): the plain-loop reference encoder on hand-derived cases,
the compressed string's round trip, the header and build entries, evaluation.CocoResults on synthetic host arrays and
pipeline.pad_annotations(with_image_ids=True).  No GPU."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

import _rle_ref as RL

ROOT = Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------------------------------------------------------------
# the reference, by hand
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask,counts", [
    ([[0, 1], [1, 1]], [1, 3]),                      # column-major pixels 0 1 1 1
    ([[1, 0], [0, 0]], [0, 1, 3]),                   # pixel 0 set: the first run of zeros is empty
    (np.zeros((3, 5), int), [15]),
    (np.ones((3, 5), int), [0, 15]),
])
def test_reference_on_hand_derived_cases(mask, counts):
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    assert RL.rle_encode(mask) == counts
    assert len(counts) == 1 + int(np.count_nonzero(np.diff(np.concatenate([[False], mask.flatten(order="F")])))) and sum(counts) == h * w
    assert np.array_equal(RL.counts_to_mask(counts, h, w), mask)
    # through the kernels' layout, with garbage outside the image: the reference reads the image's own pixels only
    packed = RL.pack(mask, h + 2, 2, fill=np.full((h + 2, 2), 0xFFFFFFFFFFFFFFFF, np.uint64))
    assert RL.encode_bits(packed, h, w) == counts and RL.encode_bits(packed.view(np.int64), h, w) == counts


def test_hand_derived_string():
    from boosted_detr_amd import pipeline
    assert pipeline.encode_rle_counts(RL.rle_encode(np.asarray([[0, 1], [1, 1]], bool))) == "13"
    assert pipeline.decode_rle_counts("13").tolist() == [1, 3]


def test_compressed_string_round_trip_on_reference_outputs():
    from boosted_detr_amd import pipeline
    rng = np.random.default_rng(27)
    seen_long, seen_negative_difference = False, False
    cases = [rng.random((h, w)) < d for (h, w) in [(1, 1), (5, 65), (37, 130), (300, 70)] for d in (0.01, 0.5, 0.99)]
    big = np.zeros((400, 300), bool)                 # runs above 2^15, and a fourth count far below the second (a negative difference)
    big[:, 100:250] = True
    big[7, 3] = big[8, 3] = True
    cases += [big, ~big]
    for mask in cases:
        counts = RL.rle_encode(mask)
        text = pipeline.encode_rle_counts(counts)
        assert isinstance(text, str) and all(48 <= ord(ch) < 112 for ch in text)
        assert pipeline.decode_rle_counts(text).tolist() == counts
        seen_long |= max(counts) > 1 << 15
        seen_negative_difference |= any(counts[i] < counts[i - 2] for i in range(3, len(counts)))
    assert seen_long and seen_negative_difference


# ---------------------------------------------------------------------------------------------------------------------
# header and build
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_both_symbols_and_the_build_lists_the_source():
    from boosted_detr_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "bdetr.h").read_text(), flags=re.S)
    for name in ("bdetr_mask_rle_count", "bdetr_mask_rle_encode"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
    assert "maskrle.hip" in build.SOURCES and (build.CSRC / "maskrle.hip").is_file()
    doc = (ROOT / "include" / "bdetr.h").read_text()
    assert "K27" in doc and "K28" in doc and "p = x h + y" in doc


# ---------------------------------------------------------------------------------------------------------------------
# CocoResults on host arrays
# ---------------------------------------------------------------------------------------------------------------------
VOCAB = ["cat", "dog", "emu"]


def _host_batch(seed, B=2, N=3, sizes=((4, 6), (3, 70))):
    rng = np.random.default_rng(seed)
    score = rng.choice([0.125, 0.25, 0.5, 0.75], (B, N)).astype(np.float32)
    score[0, 1] = 0.5
    label = rng.integers(2, 2 + len(VOCAB), (B, N)).astype(np.int32)
    box = rng.random((B, N, 4)).astype(np.float32)
    hw = np.asarray(sizes, np.int32)
    masks = [[rng.random((h, w)) < 0.4 for _ in range(N)] for (h, w) in sizes]
    return score, label, box, hw, masks


def _encoded(masks, keep=None):
    lists = [RL.rle_encode(m) if keep is None or keep[b][n] else [] for b, per in enumerate(masks) for n, m in enumerate(per)]
    return (np.asarray([v for c in lists for v in c], np.int32), np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int64))


def test_coco_results_entries_order_and_fields():
    from boosted_detr_amd import pipeline
    from boosted_detr_amd.evaluation import CocoResults
    res = CocoResults(VOCAB, {"cat": 17, "dog": 18, "emu": 90, "unused": 1})
    batches = [_host_batch(1), _host_batch(2)]
    ids = [[101, 102], ["a", 7]]
    for (score, label, box, hw, masks), image_ids in zip(batches, ids):
        res.update_from(score, label, box, image_ids, hw, *_encoded(masks))
    entries = res.result()
    assert len(entries) == 2 * 2 * 3
    k = 0
    for (score, label, box, hw, masks), image_ids in zip(batches, ids):          # batch, image, query
        for b in range(2):
            h, w = int(hw[b, 0]), int(hw[b, 1])
            for n in range(3):
                e = entries[k]
                k += 1
                assert set(e) == {"image_id", "category_id", "score", "bbox", "segmentation"}
                assert e["image_id"] == image_ids[b] and type(e["image_id"]) in (int, str)
                assert e["category_id"] == {2: 17, 3: 18, 4: 90}[int(label[b, n])] and type(e["category_id"]) is int
                assert type(e["score"]) is float and e["score"] == float(score[b, n])
                assert e["bbox"] == [float(box[b, n, 0]) * float(w), float(box[b, n, 1]) * float(h), float(box[b, n, 2]) * float(w),
                                     float(box[b, n, 3]) * float(h)] and all(type(v) is float for v in e["bbox"])
                seg = e["segmentation"]
                assert seg["size"] == [h, w] and isinstance(seg["counts"], str)
                counts = pipeline.decode_rle_counts(seg["counts"]).tolist()
                assert counts == RL.rle_encode(masks[b][n]) and sum(counts) == h * w
    assert json.loads(json.dumps(entries)) == entries


def test_coco_results_threshold_mapping_and_plain_counts(tmp_path):
    from boosted_detr_amd.evaluation import CocoResults, category_id_table
    score, label, box, hw, masks = _host_batch(3)
    every = CocoResults(VOCAB, compress=False)
    every.update_from(score, label, box, [5, 6], hw, *_encoded(masks))
    keep = score > np.float32(0.5)                   # a score EQUAL to the threshold is dropped
    assert not keep[0, 1] and keep.any() and not keep.all()
    some = CocoResults(VOCAB, score_threshold=0.5, compress=False)
    some.update_from(score, label, box, [5, 6], hw, *_encoded(masks, keep))      # unkept masks have an empty span
    flat = [e for e, k in zip(every.result(), keep.reshape(-1)) if k]
    assert some.result() == flat and len(flat) == int(keep.sum())
    assert all(e["category_id"] == int(l) - 2 for e, l in zip(every.result(), label.reshape(-1)))            # None: the id is l - 2
    assert all(isinstance(e["segmentation"]["counts"], list) and all(type(v) is int for v in e["segmentation"]["counts"]) for e in flat)
    boxes_only = CocoResults(VOCAB, score_threshold=0.5)
    boxes_only.update_from(score, label, box, np.asarray([5, 6]), hw)
    assert [{k: v for k, v in e.items() if k != "segmentation"} for e in flat] == boxes_only.result()
    assert all(type(e["image_id"]) is int for e in boxes_only.result())
    path = tmp_path / "results.json"
    some.dump(path)
    assert json.loads(path.read_text()) == flat
    some.reset()
    assert some.result() == []
    categories = [{"id": 3, "name": "dog", "supercategory": "x"}, {"id": 1, "name": "cat"}, {"id": 9, "name": "emu"}]
    assert category_id_table(VOCAB, categories) == [1, 3, 9] and category_id_table(VOCAB) == [0, 1, 2]


def test_coco_results_refusals():
    from boosted_detr_amd.evaluation import CocoResults, batch_image_ids
    with pytest.raises(ValueError, match="emu"):
        CocoResults(VOCAB, {"cat": 1, "dog": 2})
    with pytest.raises(ValueError, match="categories"):
        CocoResults(VOCAB, [1, 2, 3])
    with pytest.raises(ValueError, match="image_id"):
        batch_image_ids({"image": None})
    assert batch_image_ids({"image_id": np.asarray([3, 4])}) == [3, 4] and batch_image_ids({"image_id": ("a", 2)}) == ["a", 2]
    score, label, box, hw, masks = _host_batch(4)
    res = CocoResults(VOCAB)
    with pytest.raises(ValueError, match="image_ids"):
        res.update_from(score, label, box, [1], hw)
    with pytest.raises(ValueError, match="offset"):
        res.update_from(score, label, box, [1, 2], hw, np.zeros(3, np.int32), np.asarray([0, 5, 2, 3, 3, 3, 3]))
    counts, offset = _encoded(masks, np.zeros((2, 3), bool))
    with pytest.raises(ValueError, match="no run lengths"):
        res.update_from(score, label, box, [1, 2], hw, counts, offset)
    bad = label.copy()
    bad[0, 0] = 1
    with pytest.raises(ValueError, match="labels"):
        res.update_from(score, bad, box, [1, 2], hw)
    with pytest.raises(ValueError, match="max_mask_bytes"):
        CocoResults(VOCAB, max_mask_bytes=100).check_batch([1, 2], hw, 2, 3, True)
    assert CocoResults(VOCAB, max_mask_bytes=100).check_batch([1, 2], hw, 2, 3, False)[1:] == (0, 0)


def test_model_method_exists_with_the_documented_signature():
    import inspect
    from boosted_detr_amd.training import Model
    p = inspect.signature(Model.coco_results).parameters
    assert list(p) == ["self", "x", "steps", "iou_types", "score_threshold", "category_ids", "compress", "path"]
    assert p["iou_types"].default == ("bbox",) and p["score_threshold"].default is None and p["compress"].default is True


# ---------------------------------------------------------------------------------------------------------------------
# pad_annotations
# ---------------------------------------------------------------------------------------------------------------------
def test_pad_annotations_image_ids():
    from boosted_detr_amd import pipeline
    records = [{"image_id": 42, "bbox": [[0.1, 0.1, 0.2, 0.2]], "category": [["cat"]], "height": 4, "width": 6, "iscrowd": [0], "area": [3.0],
                "segmentation": [[[1.0, 1.0, 3.0, 1.0, 3.0, 3.0]]]},
               {"image_id": "b", "bbox": [], "category": [], "height": 3, "width": 70, "iscrowd": [], "area": [], "segmentation": []}]
    for kw in ({}, {"with_eval_fields": True}, {"with_eval_fields": True, "with_masks": True}):
        plain = pipeline.pad_annotations(records, **kw)
        with_ids = pipeline.pad_annotations(records, with_image_ids=True, **kw)
        assert "image_id" not in plain and set(with_ids) == set(plain) | {"image_id"}          # the default output keeps its keys
        assert with_ids["image_id"] == [42, "b"]
        for k in plain:
            if k != "segments":
                assert np.array_equal(plain[k], with_ids[k]), k
    assert set(pipeline.pad_annotations(records)) == {"category", "attribute", "bbox", "num_objects"}
    with pytest.raises(ValueError, match="image_id"):
        pipeline.pad_annotations([{"bbox": [], "category": []}], with_image_ids=True)
