"""CPU half of the mask-target rasteriser (K18): the RLE codec, the plain-loop reference's own consistency, the host packing in
pipeline.py, the ABI declarations and the wrapper's validation.  Nothing here needs a GPU.

The three codec vectors were made with a scratch restatement of the public COCO compressed-RLE description, NOT with pycocotools
(which is not available to this project); _mask_raster_ref.decode / encode are a second restatement of the same description."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

import _mask_raster_ref as R

ROOT = Path(__file__).resolve().parent.parent

CODEC_VECTORS = [([6, 1, 40, 4, 5, 4, 5, 4, 21], "61X13mN000`0"),
                 ([0, 3, 100, 2000, 7, 1, 40000, 5], "03T3]n1SMaQNiQW14"),
                 ([272, 2, 4, 4, 4, 4, 2, 9], "`824200N5")]

PLACEMENTS = [R.DEFAULT_PLACEMENT, (96, 96, 96, 96, 0, 0), (96, 96, 50, 77, 46, 19), (64, 80, 40, 43, 0, 37)]


# ---------------------------------------------------------------- codec
@pytest.mark.parametrize("counts,text", CODEC_VECTORS)
def test_codec_vectors_both_ways(counts, text):
    from boosted_detr_amd import pipeline
    got = pipeline.decode_rle_counts(text)
    assert got.dtype == np.int64 and got.tolist() == counts
    assert pipeline.decode_rle_counts(text.encode("ascii")).tolist() == counts
    assert pipeline.decode_rle_counts(counts).tolist() == counts and pipeline.decode_rle_counts(counts).dtype == np.int64
    assert pipeline.encode_rle_counts(counts) == text
    assert R.decode(text) == counts and R.encode(counts) == text


def test_codec_round_trip_random():
    from boosted_detr_amd import pipeline
    rng = np.random.default_rng(5)
    for _ in range(20):
        counts = rng.integers(0, 3000, rng.integers(1, 60)).tolist()
        assert pipeline.decode_rle_counts(pipeline.encode_rle_counts(counts)).tolist() == counts


def test_bad_counts_raise():
    from boosted_detr_amd import pipeline
    with pytest.raises(ValueError, match="negative"):
        pipeline.decode_rle_counts([3, -1, 4])
    with pytest.raises(ValueError, match="negative"):
        pipeline.decode_rle_counts(pipeline.encode_rle_counts([3, -2]))
    with pytest.raises(ValueError, match="ends inside"):
        pipeline.decode_rle_counts("61X")                      # 'X' has the continuation bit set
    with pytest.raises(ValueError, match="alphabet"):
        pipeline.decode_rle_counts("6 1")
    with pytest.raises(ValueError, match="integers"):
        pipeline.decode_rle_counts([1.5, 2.5])
    with pytest.raises(ValueError, match="alphabet"):
        pipeline.decode_rle_counts("6\u00e91")                 # non-ASCII: refused, never mapped to a character inside the alphabet
    rec = {"height": 4, "width": 8, "bbox": [[0, 0, 1, 1]], "category": [["cat"]]}
    with pytest.raises(ValueError, match="sum to"):
        pipeline.pad_annotations([dict(rec, segmentation=[{"size": [4, 8], "counts": [4, 8, 19]}])], with_masks=True)
    with pytest.raises(ValueError, match="differs from the image"):
        pipeline.pad_annotations([dict(rec, segmentation=[{"size": [8, 4], "counts": [4, 8, 20]}])], with_masks=True)
    with pytest.raises(ValueError, match="4096"):
        pipeline.pad_annotations([dict(rec, width=4097, segmentation=[[[0, 0, 1, 0, 1, 1]]])], with_masks=True)
    with pytest.raises(ValueError, match="2\\^23"):
        pipeline.pad_annotations([dict(rec, segmentation=[[[0, 0, 40000, 0, 1, 1]]])], with_masks=True)
    with pytest.raises(ValueError, match="with_masks=True"):
        pipeline.pad_annotations([rec], with_masks=True)       # records made without the flag
    seg = pipeline.pad_annotations([dict(rec, segmentation=[None])], with_masks=True)
    with pytest.raises(ValueError, match="placement values"):
        pipeline.mask_targets(seg, placement=(2 ** 32 + 96, 96, 96, 96, 0, 0))      # would wrap to 96 in int32
    with pytest.raises(ValueError, match="6 integers"):
        pipeline.mask_targets(seg, placement=[[1, 1, 1, 1, 0, 0]] * 2)
    with pytest.raises(ValueError, match="odd number"):
        pipeline.pad_annotations([dict(rec, segmentation=[[[0, 0, 1, 0, 1]]])], with_masks=True)


# ---------------------------------------------------------------- the reference's own consistency
def test_reference_rectangle_with_integer_corners():
    for (h, w, x0, y0, x1, y1) in [(7, 9, 2, 1, 6, 5), (5, 5, 0, 0, 5, 5), (8, 8, 3, 3, 4, 4), (6, 10, -2, -1, 4, 9)]:
        m = R.polygon_mask([[x0, y0, x1, y0, x1, y1, x0, y1]], h, w)
        want = np.zeros((h, w), bool)
        want[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = True
        assert np.array_equal(m, want), (h, w, x0, y0, x1, y1)


def _star(h, w, n, rng):
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rad = rng.uniform(0.15, 0.65, n) * min(h, w)
    return np.stack([w / 2 + rad * np.cos(ang), h / 2 + rad * np.sin(ang)], axis=-1).reshape(-1).tolist()


@pytest.mark.parametrize("G", [23, 4])
def test_reference_total_weight_and_polygon_equals_its_rle(G):
    rng = np.random.default_rng(11)
    for (h, w) in [(1, 1), (5, 20), (37, 53)]:
        mask = R.polygon_mask([_star(h, w, 12, rng)], h, w)
        if h == 1:
            mask[:] = True
        counts = R.mask_to_counts(mask)
        assert sum(counts) == h * w and np.array_equal(R.rle_mask(counts, h, w), mask)
        assert np.array_equal(R.rle_mask(R.decode(R.encode(counts)), h, w), mask)
        for pl in PLACEMENTS:
            N = R.numerator(mask, G, pl)
            assert N.dtype == np.int64 and int(N.sum()) == int(mask.sum()) * G * pl[2] * G * pl[3]
            assert np.array_equal(N, R.numerator(R.rle_mask(counts, h, w), G, pl))
            t, area = R.target(mask, G, pl)
            assert t.dtype == np.float32 and t.min() >= 0.0 and t.max() <= 1.0 and area == int(mask.sum())
    # a mask that fills the source fills exactly the placed rectangle: cells inside it are 1
    t, _ = R.target(np.ones((7, 5), bool), 4, (96, 96, 48, 96, 48, 0))
    assert np.array_equal(t, np.repeat(np.asarray([[0], [0], [1], [1]], np.float32), 4, axis=1))


def test_reference_known_answers():
    kats = json.loads((ROOT / "tests" / "golden" / "mask_raster_kats.json").read_text())
    assert "BY HAND" in kats["note"] and {c["name"] for c in kats["cases"]} >= {"bowtie", "nested"}
    for c in kats["cases"]:
        assert c["h"] <= 8 and c["w"] <= 8
        want = np.asarray([[ch == "1" for ch in row] for row in c["mask"]])
        assert want.shape == (c["h"], c["w"])
        assert np.array_equal(R.polygon_mask(c["rings"], c["h"], c["w"]), want), c["name"]


# ---------------------------------------------------------------- pipeline
COCO = {"images": [{"id": 1, "file_name": "a.jpg", "width": 8, "height": 4}, {"id": 2, "width": 4, "height": 4}],
        "categories": [{"id": 5, "name": "cat"}, {"id": 7, "name": "dog"}],
        "annotations": [{"image_id": 1, "category_id": 5, "bbox": [2, 1, 4, 2], "iscrowd": 0, "area": 8,
                         "segmentation": [[2, 1, 6, 1, 6, 3, 2, 3]]},
                        {"image_id": 1, "category_id": 7, "bbox": [0, 0, 8, 4], "iscrowd": 1,
                         "segmentation": {"size": [4, 8], "counts": [4, 8, 20]}},
                        {"image_id": 2, "category_id": 5, "bbox": [1, 1, 2, 2]}]}


def test_defaults_are_unchanged():
    from boosted_detr_amd import pipeline
    recs = pipeline.coco_records(COCO)
    assert recs == [{"image_id": 1, "file_name": "a.jpg", "width": 8, "height": 4, "category": [["cat"], ["dog"]],
                     "attribute": [["<PAD>"], ["<PAD>"]], "bbox": [[0.25, 0.25, 0.5, 0.5], [0.0, 0.0, 1.0, 1.0]]},
                    {"image_id": 2, "file_name": "", "width": 4, "height": 4, "category": [["cat"]], "attribute": [["<PAD>"]],
                     "bbox": [[0.25, 0.25, 0.5, 0.5]]}]
    out = pipeline.pad_annotations(recs)
    assert set(out) == {"category", "attribute", "bbox", "num_objects"}
    assert out["category"].tolist() == [[["cat"], ["dog"]], [["cat"], ["<PAD>"]]]
    assert out["attribute"].tolist() == [[["<PAD>"], ["<PAD>"]], [["<PAD>"], ["<PAD>"]]]
    assert out["bbox"].dtype == np.float32 and out["bbox"].tolist() == [[[0.25, 0.25, 0.5, 0.5], [0, 0, 1, 1]], [[0.25, 0.25, 0.5, 0.5], [-10] * 4]]
    assert out["num_objects"].dtype == np.int32 and out["num_objects"].tolist() == [2, 1]
    ev = pipeline.pad_annotations(pipeline.coco_records(COCO, with_eval_fields=True), with_eval_fields=True)
    assert set(ev) == set(out) | {"iscrowd", "area", "height", "width"} and ev["area"].tolist() == [[8.0, 32.0], [4.0, 0.0]]


def test_with_masks_packs_the_segmentations():
    from boosted_detr_amd import pipeline
    from boosted_detr_amd import kernels as K
    recs = pipeline.coco_records(COCO, with_masks=True)
    plain = pipeline.coco_records(COCO)
    assert [{k: v for k, v in r.items() if k != "segmentation"} for r in recs] == plain
    assert recs[0]["segmentation"] == [[[2, 1, 6, 1, 6, 3, 2, 3]], {"size": [4, 8], "counts": [4, 8, 20]}] and recs[1]["segmentation"] == [None]
    out = pipeline.pad_annotations(recs, with_masks=True)
    base = pipeline.pad_annotations(plain)
    assert set(out) == set(base) | {"segments"} and all(np.array_equal(out[k], base[k]) for k in base)
    seg = out["segments"]
    assert set(seg) == {"items", "item_off", "kind", "hw"} and all(v.dtype == np.int32 for v in seg.values())
    assert seg["kind"].tolist() == [[1, 2], [0, 0]]
    assert seg["hw"].tolist() == [[[4, 8], [4, 8]], [[4, 4], [0, 0]]]
    assert seg["item_off"].tolist() == [0, 11, 13, 13, 13]
    assert seg["items"].tolist() == [1, 0, 4, 512, 256, 1536, 256, 1536, 768, 512, 768, 4, 8]
    assert K.check_mask_pack(seg["items"], seg["item_off"], seg["kind"], seg["hw"], np.tile(np.asarray([[1, 1, 1, 1, 0, 0]], np.int32), (2, 1)), 23) == (2, 2)
    # the compressed string packs to the same runs; zero-length one-runs are dropped; truncation follows bbox
    text = dict(recs[0], segmentation=[recs[0]["segmentation"][0], {"size": [4, 8], "counts": pipeline.encode_rle_counts([4, 8, 20])}])
    assert np.array_equal(pipeline.pad_annotations([text], with_masks=True)["segments"]["items"], seg["items"])
    zero = dict(recs[0], segmentation=[None, {"size": [4, 8], "counts": [0, 3, 5, 0, 2, 22]}])
    assert pipeline.pad_annotations([zero], with_masks=True)["segments"]["items"].tolist() == [0, 3, 10, 22]
    cut = pipeline.pad_annotations(recs, max_objects=1, with_masks=True)
    assert cut["segments"]["kind"].tolist() == [[1], [0]] and cut["segments"]["item_off"].tolist() == [0, 11, 11] and cut["bbox"].shape == (2, 1, 4)
    # snapping is round-half-to-even on 1/256 pixel
    half = dict(recs[0], segmentation=[[[0.001953125, 0.005859375, 1, 0, 1, 1]], None])       # 0.5 / 256 -> 0, 1.5 / 256 -> 2
    assert pipeline.pad_annotations([half], with_masks=True)["segments"]["items"][3:5].tolist() == [0, 2]


# ---------------------------------------------------------------- ABI and validation
def test_new_symbol_is_declared_bound_and_exported():
    import ctypes as C
    from boosted_detr_amd import _lib, build, kernels, pipeline
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "bdetr.h").read_text(), flags=re.S)
    decl = re.search(r"\bint\s+bdetr_mask_targets\s*\(([^)]*)\)", header)
    assert decl, "bdetr_mask_targets is not declared in include/bdetr.h"
    kinds = []
    for arg in decl.group(1).split(","):
        arg = arg.strip()
        kinds.append(C.c_void_p if "*" in arg else C.c_int64 if arg.startswith("int64_t") else C.c_int)
    res, args = _lib.SIGNATURES["bdetr_mask_targets"]
    assert res is C.c_int and args == kinds
    assert "maskraster.hip" in build.SOURCES and "-ffp-contract=off" in build.PER_FILE_FLAGS["maskraster.hip"]
    assert callable(kernels.mask_targets) and callable(pipeline.mask_targets) and callable(pipeline.decode_rle_counts)
    import __graft_entry__
    __graft_entry__.build()
    h = _lib.lib()
    assert h.bdetr_abi_version() == 8 and hasattr(h, "bdetr_mask_targets")
    # the entry refuses bad sizes without a launch (no GPU is touched)
    assert h.bdetr_mask_targets(None, 0, 1, 1, 1, 1, 1, 1, 33, 1, 1, None) == -1
    assert b"G in [1, 32]" in h.bdetr_last_error()
    assert h.bdetr_mask_targets(None, 0, None, 1, 1, 1, 1, 1, 23, 1, 1, None) == -1 and b"null pointer" in h.bdetr_last_error()


def test_wrapper_validation_raises_before_any_launch():
    from boosted_detr_amd import _lib
    from boosted_detr_amd import kernels as K
    good = dict(items=np.asarray([1, 0, 3, 0, 0, 256, 0, 256, 256, 0, 4], np.int32), item_off=np.asarray([0, 9, 11], np.int32),
                kind=np.asarray([[1, 2]], np.int32), hw=np.asarray([[[4, 8], [4, 8]]], np.int32),
                placement=np.asarray([[96, 96, 50, 77, 46, 19]], np.int32), grid=23)
    assert K.check_mask_pack(**good) == (1, 2)

    def bad(exc, match, **change):
        with pytest.raises(exc, match=match):
            K.mask_targets(**dict(good, **change))

    bad(_lib.BdetrError, "items must be an int32", items=good["items"].astype(np.int64))
    bad(_lib.BdetrError, "hw must be an int32", hw=good["hw"].astype(np.float32))
    bad(_lib.BdetrError, "placement must be an int32", placement=[[1, 1, 1, 1, 0, 0]])
    bad(_lib.BdetrError, "shapes disagree", item_off=np.asarray([0, 9], np.int32))
    bad(_lib.BdetrError, "shapes disagree", placement=np.asarray([[1, 1, 1, 1, 0, 0]] * 2, np.int32))
    bad(ValueError, "non-decreasing", item_off=np.asarray([0, 11, 9], np.int32))
    bad(ValueError, "inside the item buffer", item_off=np.asarray([0, 9, 12], np.int32))
    bad(ValueError, "non-decreasing", item_off=np.asarray([-1, 9, 11], np.int32))
    bad(ValueError, "4096", hw=np.asarray([[[4, 4097], [4, 8]]], np.int32))
    bad(ValueError, "4096", hw=np.asarray([[[0, 8], [4, 8]]], np.int32))
    bad(ValueError, "kind must be", kind=np.asarray([[1, 3]], np.int32))
    bad(ValueError, "grid must be", grid=33)
    bad(ValueError, "off \\+ new <= canvas", placement=np.asarray([[96, 96, 51, 77, 46, 19]], np.int32))
    bad(ValueError, "off \\+ new <= canvas", placement=np.asarray([[96, 4097, 50, 77, 46, 19]], np.int32))
    bad(ValueError, "ring offsets", items=np.asarray([1, 0, 4, 0, 0, 256, 0, 256, 256, 0, 4], np.int32))
    bad(ValueError, "2\\^23", items=np.asarray([1, 0, 3, 0, 0, (1 << 23) + 1, 0, 256, 256, 0, 4], np.int32))
    bad(ValueError, "one-runs", items=np.asarray([1, 0, 3, 0, 0, 256, 0, 256, 256, 30, 4], np.int32))      # runs past h * w
    bad(ValueError, "one-runs", items=np.asarray([1, 0, 3, 0, 0, 256, 0, 256, 256, 0, -4], np.int32))
    two = dict(good, items=np.asarray([1, 0, 3, 0, 0, 256, 0, 256, 256, 5, 4, 8, 2], np.int32), item_off=np.asarray([0, 9, 13], np.int32))
    with pytest.raises(ValueError, match="one-runs"):
        K.mask_targets(**two)                                                                          # overlapping runs
