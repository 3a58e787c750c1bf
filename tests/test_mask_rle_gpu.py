"""GPU half of the COCO result-file export (csrc/maskrle.hip): bdetr_mask_rle_count (K27) and bdetr_mask_rle_encode (K28) bit for bit
against the plain-loop reference (tests/_rle_ref.py), the round trip through the existing decoder and K20, and
Model.coco_results end to end."""
import functools
import json

import numpy as np
import pytest
import torch

import _mask_image_ref as MI
import _rle_ref as RL

pytestmark = pytest.mark.gpu

DEV = "cuda"
# one row, one column of words, a word boundary from both sides, three words, the widest and the tallest layout, several row blocks
SIZES = [(1, 1), (1, 130), (5, 63), (5, 64), (5, 65), (7, 130), (2, 4096), (4096, 3), (300, 70)]
MASKS = ("zero", "one", "first", "last", "checker0", "checker1", "continues", "random_0.01", "random_0.5", "random_0.99")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def make_mask(name, h, w, rng):
    y, x = np.mgrid[0:h, 0:w]
    if name == "zero":
        return np.zeros((h, w), bool)
    if name == "one":
        return np.ones((h, w), bool)
    if name == "first":
        return (y == 0) & (x == 0)
    if name == "last":
        return (y == h - 1) & (x == w - 1)
    if name.startswith("checker"):
        return (x + y) % 2 == int(name[-1])
    if name == "continues":                          # runs from the last rows of column x into the first rows of column x + 1
        m = np.zeros((h, w), bool)
        for c in sorted({0, 62, 63, 64, 127, w - 2} & set(range(w - 1))):
            m[max(h - 2, 0):, c] = True
            m[:min(2, h), c + 1] = True
        return m
    return rng.random((h, w)) < float(name.split("_")[1])


@functools.lru_cache(maxsize=None)
def mixed_batch(sizes=tuple(SIZES)):
    """(masks[b][n] bool [h, w], image_hw, clean bits, bits with garbage outside every image, the reference's (counts, offset, lists)).
    The reference reads the garbage-filled words: it looks at the image's own pixels only."""
    rng = np.random.default_rng(28)
    hw = np.asarray(sizes, np.int32)
    Hm, Wm = MI.layout(hw)
    garbage = rng.integers(0, 1 << 63, (Hm, Wm), dtype=np.int64).view(np.uint64) * np.uint64(2) + np.uint64(1)
    masks = [[make_mask(name, h, w, rng) for name in MASKS] for (h, w) in sizes]
    clean = np.stack([np.stack([RL.pack(m, Hm, Wm) for m in per]) for per in masks])
    dirty = np.stack([np.stack([RL.pack(m, Hm, Wm, fill=np.roll(garbage, n, axis=0)) for n, m in enumerate(per)]) for per in masks])
    want = RL.encode_batch(dirty, hw)
    assert all(want[2][b * len(MASKS) + n] == RL.rle_encode(m) for b in (0, len(sizes) - 1) for n, m in enumerate(masks[b]))
    return masks, hw, clean, dirty, want


def encode(bits, hw, keep=None, **kw):
    from boosted_detr_amd import kernels as K
    counts, offset = K.mask_rle_encode(dev(bits.view(np.int64)), dev(hw), None if keep is None else dev(keep.astype(np.uint8)), **kw)
    torch.cuda.synchronize()
    return counts, offset


def assert_equal_to(want, counts, offset, what):
    want_counts, want_offset, lists = want
    assert counts.dtype == torch.int32 and offset.dtype == torch.int64 and counts.is_cuda and offset.is_cuda
    got_offset, got = offset.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(got_offset, want_offset), (what, np.flatnonzero(got_offset != want_offset)[:4].tolist())
    for o, c in enumerate(lists):
        assert got[got_offset[o]:got_offset[o + 1]].tolist() == c, (what, divmod(o, len(MASKS)))
    assert np.array_equal(got, want_counts), what


def test_encode_bit_for_bit_mixed_sizes_and_garbage_outside_the_image(cuda):
    from boosted_detr_amd import kernels as K
    masks, hw, clean, dirty, want = mixed_batch()
    Hm, Wm = clean.shape[2:]
    assert (Hm, Wm) == (4096, 64) and any(h < Hm for h, _ in SIZES) and any(w < 64 * Wm for _, w in SIZES)
    assert clean[0, 1].sum() == 1 and (dirty[0, 1] != clean[0, 1]).sum() > Hm * Wm // 2          # the garbage is there
    counts, offset = encode(clean, hw)
    assert_equal_to(want, counts, offset, "clean")
    n_counts = K.mask_rle_count(dev(clean.view(np.int64)), dev(hw))
    assert n_counts.dtype == torch.int32 and np.array_equal(n_counts.cpu().numpy().reshape(-1), np.diff(want[1]))
    # the hand-derived properties on what came back
    lists = want[2]
    for b, (h, w) in enumerate(SIZES):
        row = lists[b * len(MASKS):(b + 1) * len(MASKS)]
        assert row[0] == [h * w] and row[1] == [0, h * w] and all(sum(c) == h * w for c in row)
        assert row[2] == ([0, 1, h * w - 1] if h * w > 1 else [0, 1]) and row[3] == ([h * w - 1, 1] if h * w > 1 else [0, 1])
        if h % 2:                                    # an odd height: the checkerboard alternates across the column ends too
            assert row[4] == [0] + [1] * (h * w) and row[5] == [1] * (h * w)
    dirty_counts, dirty_offset = encode(dirty, hw)   # bits at x >= w and rows y >= h change nothing
    assert_equal_to(want, dirty_counts, dirty_offset, "garbage")
    assert torch.equal(dirty_counts, counts) and torch.equal(dirty_offset, offset)
    again_counts, again_offset = encode(dirty, hw)   # a pure function of the input
    assert torch.equal(again_counts, counts) and torch.equal(again_offset, offset)


def test_odd_word_count_takes_the_narrow_loads(cuda):
    """Wm = 3: 8-byte loads in K27 (Wm = 64 above takes the 16-byte ones); Hm > every h."""
    sizes = ((5, 65), (7, 130), (300, 70), (64, 129))
    masks, hw, clean, dirty, want = mixed_batch(sizes)
    assert clean.shape[2:] == (300, 3)
    for bits, what in ((clean, "clean"), (dirty, "garbage")):
        counts, offset = encode(bits, hw)
        assert_equal_to(want, counts, offset, what)
    taller = np.concatenate([dirty, ~np.zeros((len(sizes), len(MASKS), 5, 3), np.uint64)], axis=2)      # another batch's Hm
    counts, offset = encode(taller, hw)
    assert_equal_to(want, counts, offset, "taller layout")


def test_keep(cuda):
    from boosted_detr_amd import kernels as K
    masks, hw, clean, dirty, want = mixed_batch()
    B, N = len(SIZES), len(MASKS)
    keep = (np.arange(B * N).reshape(B, N) * 7 % 3 != 0)
    assert keep.any() and not keep.all()
    lists = [c if k else [] for c, k in zip(want[2], keep.reshape(-1))]
    want_kept = (np.asarray([v for c in lists for v in c], np.int32), np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int64), lists)
    counts, offset = encode(dirty, hw, keep)         # unkept masks: an empty span; the others do not see their neighbours
    assert_equal_to(want_kept, counts, offset, "keep")
    n_counts = K.mask_rle_count(dev(dirty.view(np.int64)), dev(hw), dev(keep.astype(np.uint8)))
    assert np.array_equal(n_counts.cpu().numpy(), np.where(keep, np.diff(want[1]).reshape(B, N), 0))
    counts, offset = encode(dirty, hw, np.zeros((B, N), bool))
    assert counts.numel() == 0 and counts.dtype == torch.int32 and not offset.any() and offset.numel() == B * N + 1
    total = int(want[1][-1])
    with pytest.raises(ValueError, match="max_bytes"):
        encode(dirty, hw, max_bytes=4 * total - 1)
    counts, offset = encode(dirty, hw, max_bytes=4 * total)
    assert counts.numel() == total


def test_operand_checks_refuse_before_a_launch(cuda):
    from boosted_detr_amd import _lib
    from boosted_detr_amd import kernels as K
    bits, hw = torch.zeros(2, 3, 4, 1, dtype=torch.int64, device=DEV), torch.ones(2, 2, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.BdetrError, match="bits"):
        K.mask_rle_encode(bits.to(torch.int32), hw)
    with pytest.raises(_lib.BdetrError, match="image_hw"):
        K.mask_rle_encode(bits, hw[:1])
    with pytest.raises(_lib.BdetrError, match="keep"):
        K.mask_rle_count(bits, hw, torch.ones(2, 4, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="Wm"):
        K.mask_rle_count(torch.zeros(1, 1, 2, 65, dtype=torch.int64, device=DEV), hw[:1])
    with pytest.raises(_lib.BdetrError, match="HBM"):
        K.mask_rle_count(bits.cpu(), hw.cpu())


def test_round_trip_through_the_decoder_and_k20(cuda):
    """counts -> RLE dicts (lists and compressed strings) -> pad_annotations(with_masks=True) -> bdetr_mask_source_bits: the input
    words again, and pop their popcount."""
    from boosted_detr_amd import kernels as K
    from boosted_detr_amd import pipeline
    sizes = ((5, 65), (7, 130), (300, 70), (64, 129))
    masks, hw, clean, _, _ = mixed_batch(sizes)
    Hm, Wm = clean.shape[2:]
    counts, offset = encode(clean, hw)
    got, off = counts.cpu().numpy(), offset.cpu().numpy()
    N = len(MASKS)
    records = []
    for b, (h, w) in enumerate(sizes):
        runs = [got[off[b * N + n]:off[b * N + n + 1]].tolist() for n in range(N)]
        segs = [{"size": [h, w], "counts": pipeline.encode_rle_counts(c) if n % 2 else c} for n, c in enumerate(runs)]
        records.append({"height": h, "width": w, "segmentation": segs, "bbox": [[0.0, 0.0, 1.0, 1.0]] * N, "category": [["x"]] * N})
    pack = pipeline.pad_annotations(records, with_masks=True)["segments"]
    bits, pop = K.mask_source_bits(pack["items"], pack["item_off"], pack["kind"], pack["hw"], Hm, Wm)
    torch.cuda.synchronize()
    assert np.array_equal(bits.cpu().numpy().view(np.uint64), clean)
    assert np.array_equal(pop.cpu().numpy(), np.asarray([[int(m.sum()) for m in per] for per in masks]))


# ---------------------------------------------------------------------------------------------------------------------
# model level: the small head model of tests/test_panoptic_train_gpu.py (64 x 64 inputs, 30 queries); the images' sizes differ
# ---------------------------------------------------------------------------------------------------------------------
ORIGINAL = [[(48, 80), (100, 60)], [(64, 64), (33, 130)]]          # per batch, per image: (height, width)
IMAGE_IDS = [[397133, 37777], [252219, "val-87038"]]


@pytest.fixture(scope="module")
def trained(cuda):
    from boosted_detr_amd import kernels as K
    from boosted_detr_amd.training import SGD
    from test_panoptic_train_gpu import _small_head_batch, _small_head_model
    prev = K.set_deterministic(True)                 # segmentations() below repeats coco_results' forward passes: the same bits
    try:
        batches = [_small_head_batch(9), _small_head_batch(21)]
        model = _small_head_model()
        model.compile(optimizer=SGD(learning_rate=1e-3, momentum=.9, nesterov=True, clipnorm=.1))
        for i in range(3):
            model.train_step(batches[i % 2])
        for i, b in enumerate(batches):
            b.update(height=np.asarray([h for h, _ in ORIGINAL[i]], np.int32), width=np.asarray([w for _, w in ORIGINAL[i]], np.int32),
                     image_id=IMAGE_IDS[i])
        torch.cuda.synchronize()
        yield batches, model
    finally:
        K.set_deterministic(prev)


def test_coco_results_end_to_end(trained, tmp_path):
    from boosted_detr_amd import kernels as K
    from boosted_detr_amd import pipeline
    from test_coco_eval_gpu import state_of
    batches, model = trained
    names = model.vocab_dict["category"]
    mapping = {name: 1000 + 7 * k for k, name in enumerate(names)}
    model.predict_raw(batches[0])                    # the user's last call
    users_masks = model.panoptic_masks().clone()
    before = state_of(model)
    path = tmp_path / "segm.json"
    entries = model.coco_results(batches, iou_types=("bbox", "segm"), category_ids=mapping, path=path)
    assert torch.equal(model.panoptic_masks(), users_masks)          # still the user's call
    scores = np.concatenate([model.detections(b)["scores"].cpu().numpy().reshape(-1) for b in batches])
    threshold = float(np.sort(scores)[scores.size // 2])
    filtered = model.coco_results(batches, iou_types=("bbox", "segm"), category_ids=mapping, score_threshold=threshold)
    plain = model.coco_results(batches, iou_types="segm", compress=False, steps=1)
    boxes = model.coco_results(batches)
    torch.cuda.synchronize()
    model.predict_raw(batches[0])
    after = state_of(model)
    assert before[1] == after[1] and set(before[0]) == set(after[0]) and len(before[0]) > 100
    for k, t in before[0].items():
        assert torch.equal(t, after[0][k]), k        # weights, moving statistics, optimizer slots: bit-identical
    assert torch.equal(model.panoptic_masks(), users_masks)

    N = model.num_object_preds
    assert len(entries) == 2 * 2 * N and len(plain) == 2 * N and json.loads(path.read_text()) == entries == json.loads(json.dumps(entries))
    k = 0
    for i, batch in enumerate(batches):
        seg = model.segmentations(batch, resolution="image")
        score, label, box = (seg[key].cpu().numpy() for key in ("scores", "labels", "boxes"))
        area = seg["image_mask_area"].cpu().numpy()
        Hm, Wm = MI.layout(ORIGINAL[i])
        records = []
        for b, (h, w) in enumerate(ORIGINAL[i]):
            segs = []
            for n in range(N):
                e = entries[k]
                k += 1
                assert set(e) == {"image_id", "category_id", "score", "bbox", "segmentation"}
                assert e["image_id"] == IMAGE_IDS[i][b] and e["category_id"] == mapping[names[int(label[b, n]) - 2]]
                assert type(e["score"]) is float and e["score"] == float(score[b, n])
                assert e["bbox"] == [float(box[b, n, 0]) * float(w), float(box[b, n, 1]) * float(h), float(box[b, n, 2]) * float(w),
                                     float(box[b, n, 3]) * float(h)]
                assert e["segmentation"]["size"] == [h, w] and isinstance(e["segmentation"]["counts"], str)
                counts = pipeline.decode_rle_counts(e["segmentation"]["counts"])
                assert int(counts.sum()) == h * w and int(counts[1::2].sum()) == int(area[b, n]), (i, b, n)
                if i == 0:
                    assert plain[b * N + n]["segmentation"] == {"size": [h, w], "counts": counts.tolist()} and plain[b * N + n]["score"] == e["score"]
                segs.append(e["segmentation"])
            records.append({"height": h, "width": w, "segmentation": segs, "bbox": [[0.0, 0.0, 1.0, 1.0]] * N, "category": [["x"]] * N})
        pack = pipeline.pad_annotations(records, with_masks=True)["segments"]
        bits, pop = K.mask_source_bits(pack["items"], pack["item_off"], pack["kind"], pack["hw"], Hm, Wm)      # through K20
        assert torch.equal(bits, seg["image_masks"]) and torch.equal(pop, seg["image_mask_area"]), i
        assert 0 < int(pop.sum()) < sum(h * w for h, w in ORIGINAL[i]) * N
    assert k == len(entries)
    assert filtered == [e for e in entries if e["score"] > float(np.float32(threshold))] and 0 < len(filtered) < len(entries)
    assert boxes == [{key: v for key, v in e.items() if key != "segmentation"} | {"category_id": (e["category_id"] - 1000) // 7} for e in entries]

    last_call = model.panoptic_masks().clone()       # segmentations(batches[1]) above
    with pytest.raises(ValueError, match="image_id"):
        model.coco_results([{key: v for key, v in batches[0].items() if key != "image_id"}])
    with pytest.raises(ValueError, match="height"):
        model.coco_results([{key: v for key, v in batches[0].items() if key not in ("height", "width")}], iou_types="segm")
    with pytest.raises(ValueError, match="host array"):
        model.coco_results([dict(batches[0], height=torch.as_tensor(batches[0]["height"]).cuda())], iou_types="segm")
    with pytest.raises(ValueError, match="category_ids"):
        model.coco_results(batches, category_ids={names[0]: 1})
    assert torch.equal(model.panoptic_masks(), last_call)


def test_models_without_a_mask_head_export_boxes_only(cuda):
    from boosted_detr_amd import parameters
    from boosted_detr_amd.engine import to_device
    from boosted_detr_amd.model import DETR
    plain = DETR(num_object_preds=10, image_size=(64, 64), num_encoder_blocks=1, num_encoder_heads=8, encoder_dim=256, num_decoder_blocks=1,
                 num_decoder_heads=8, decoder_dim=256, vocab_dict=parameters.synthetic_vocab(10, 4))
    with pytest.raises(RuntimeError, match="with_panoptic_head=True"):
        plain.coco_results([], iou_types=("bbox", "segm"))
    rng = np.random.default_rng(5)
    batch = {"image": to_device(rng.random((2, 64, 64, 3)).astype(np.float32)), "image_id": np.asarray([11, 12])}
    entries = plain.coco_results([batch, batch], steps=1)
    det = plain.detections(batch)
    score, label, box = (det[key].cpu().numpy() for key in ("scores", "labels", "boxes"))
    assert len(entries) == 20 and json.loads(json.dumps(entries)) == entries
    for k, e in enumerate(entries):
        b, n = divmod(k, 10)
        assert e == {"image_id": 11 + b, "category_id": int(label[b, n]) - 2, "score": float(score[b, n]),
                     "bbox": [float(v) * 64.0 for v in box[b, n]]}          # no height / width: the model's image_size
