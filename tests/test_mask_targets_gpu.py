"""GPU half of the mask-target rasteriser (K18, csrc/maskraster.hip): masks and areas BIT-EQUAL to the plain-loop reference
(_mask_raster_ref.py) - every quantity is an integer up to one IEEE fp64 division - through the whole host chain
(records -> pad_annotations(with_masks=True) -> mask_targets), then Augmentations.apply and one training step at configs[0].

Every (grid, placement) case is ONE launch over all source sizes x all shapes; the reference masks are computed once per module."""
import functools

import numpy as np
import pytest
import torch

import _mask_raster_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (23, 23), (37, 53), (64, 65), (5, 200), (130, 70)]           # h x w
PLACEMENTS = [None, (96, 96, 96, 96, 0, 0), (96, 96, 50, 77, 46, 19), (64, 80, 40, 43, 0, 37)]
GRIDS = [23, 4]


# ---------------------------------------------------------------- the shapes, as functions of the source size
def _star(h, w, n, seed):
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rad = rng.uniform(0.15, 0.75, n) * min(h, w)
    return np.stack([w / 2 + rad * np.cos(ang), h / 2 + rad * np.sin(ang)], axis=-1).reshape(-1).tolist()


def polygon_cases(h, w):
    m = min(h, w) - 1
    tri = [0.11 * w, 0.07 * h, 0.93 * w, 0.31 * h, 0.42 * w, 0.96 * h]
    return {
        "triangle": [tri],
        "concave_L": [[0.1 * w, 0.1 * h, 0.5 * w, 0.1 * h, 0.5 * w, 0.6 * h, 0.9 * w, 0.6 * h, 0.9 * w, 0.9 * h, 0.1 * w, 0.9 * h]],
        "bowtie": [[0.1 * w, 0.1 * h, 0.9 * w, 0.9 * h, 0.9 * w, 0.1 * h, 0.1 * w, 0.9 * h]],
        "overlapping_rings": [[0.05 * w, 0.05 * h, 0.6 * w, 0.05 * h, 0.6 * w, 0.6 * h, 0.05 * w, 0.6 * h],
                              [0.4 * w, 0.4 * h, 0.95 * w, 0.4 * h, 0.95 * w, 0.95 * h, 0.4 * w, 0.95 * h]],
        "nested_rings": [[0.1 * w, 0.1 * h, 0.9 * w, 0.1 * h, 0.9 * w, 0.9 * h, 0.1 * w, 0.9 * h],
                         [0.3 * w, 0.3 * h, 0.7 * w, 0.3 * h, 0.7 * w, 0.7 * h, 0.3 * w, 0.7 * h]],
        "two_vertex_ring_alone": [[0.1 * w, 0.1 * h, 0.9 * w, 0.9 * h]],
        "two_vertex_ring_and_triangle": [[0.1 * w, 0.1 * h, 0.9 * w, 0.9 * h], tri],
        "outside_vertices": [[-0.7 * w, -0.3 * h, 1.8 * w, 0.4 * h, 0.3 * w, 1.9 * h]],
        "vertices_on_centres": [[0.5, 0.5, w - 0.5, 0.5, w - 0.5, h - 0.5, 0.5, h - 0.5]],
        "edge_through_centres": [[0.5, 0.5, m + 0.5, m + 0.5, 0.5, m + 0.5]],            # the diagonal passes through pixel centres
        "horizontal_on_centre_row": [[0, 0.5, w, 0.5, w, min(h, 3) - 0.5, 0.25 * w, min(h, 3) - 0.5, 0.25 * w, h, 0, h]],
        "star_200": [_star(h, w, 200, 1000 * h + w)],
    }


def _random_counts(h, w, parts, seed):
    rng = np.random.default_rng(seed)
    cuts = np.unique(rng.integers(0, h * w + 1, max(parts - 1, 0)))
    return np.diff(np.concatenate([[0], cuts, [h * w]])).tolist()


def rle_cases(h, w):
    n = h * w
    s = h // 2
    three = min(2 * h + 1, n - s)                        # from the middle of column 0 into column 2 (where the source has three)
    rnd = _random_counts(h, w, 300, 77 * h + w)
    import boosted_detr_amd.pipeline as pipeline
    return {
        "all_zeros": [n],
        "all_ones": [0, n],
        "run_over_three_columns": [c for k, c in enumerate([s, three, n - s - three]) if k < 2 or c],
        "leading_zero_length_run": [c for k, c in enumerate([0, max(n // 3, 1), n - max(n // 3, 1)]) if k < 2 or c],
        "random_300": rnd,
        "random_300_compressed": pipeline.encode_rle_counts(rnd),
    }


@functools.lru_cache(maxsize=None)
def reference_masks():
    """{(size index, name): bool [h, w]} - computed once, never modified."""
    out = {}
    for si, (h, w) in enumerate(SIZES):
        for name, rings in polygon_cases(h, w).items():
            out[si, name] = R.polygon_mask(rings, h, w)
        for name, counts in rle_cases(h, w).items():
            out[si, name] = R.rle_mask(R.decode(counts) if isinstance(counts, str) else counts, h, w)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def packed():
    """One record per source size; every shape is one object."""
    from boosted_detr_amd import pipeline
    records, names = [], None
    for (h, w) in SIZES:
        segs = dict(polygon_cases(h, w))
        segs.update({k: {"size": [h, w], "counts": c} for k, c in rle_cases(h, w).items()})
        names = list(segs)
        records.append({"height": h, "width": w, "bbox": [[0.0, 0.0, 1.0, 1.0]] * len(segs), "category": [["x"]] * len(segs),
                        "segmentation": list(segs.values())})
    return pipeline.pad_annotations(records, with_masks=True)["segments"], names


def _want(names, G, placement):
    ref = reference_masks()
    pl = R.DEFAULT_PLACEMENT if placement is None else placement
    masks = np.zeros((len(SIZES), len(names), G, G), np.float32)
    area = np.zeros((len(SIZES), len(names)), np.int32)
    for si in range(len(SIZES)):
        for m, name in enumerate(names):
            masks[si, m], area[si, m] = R.target(ref[si, name], G, pl)
    return masks, area


def _assert_bit_equal(got, want_masks, want_area, names):
    gm, ga = got["masks"].cpu().numpy(), got["mask_area"].cpu().numpy()
    assert gm.dtype == np.float32 and ga.dtype == np.int32 and gm.shape == want_masks.shape and ga.shape == want_area.shape
    for si, (h, w) in enumerate(SIZES[:gm.shape[0]]):
        for m, name in enumerate(names):
            assert ga[si, m] == want_area[si, m], (name, (h, w), int(ga[si, m]), int(want_area[si, m]))
            same = gm[si, m].view(np.uint32) == want_masks[si, m].view(np.uint32)
            assert same.all(), (name, (h, w), np.argwhere(~same)[:4].tolist(), gm[si, m][~same][:4], want_masks[si, m][~same][:4])


@pytest.mark.parametrize("placement", PLACEMENTS, ids=["default", "full96", "bottom_edge", "offset_w"])
@pytest.mark.parametrize("G", GRIDS)
def test_targets_bit_equal_to_reference(cuda, G, placement):
    from boosted_detr_amd import pipeline
    pack, names = packed()
    assert {"triangle", "bowtie", "star_200", "all_ones", "random_300_compressed"} <= set(names)
    got = pipeline.mask_targets(pack, grid=G, placement=placement)
    again = pipeline.mask_targets({"segments": pack}, grid=G, placement=placement)
    torch.cuda.synchronize()
    want_masks, want_area = _want(names, G, placement)
    assert want_area.max() > 0 and want_masks.max() == 1.0
    _assert_bit_equal(got, want_masks, want_area, names)
    assert torch.equal(got["masks"], again["masks"]) and torch.equal(got["mask_area"], again["mask_area"])      # determinism
    assert got["masks"].is_cuda and tuple(got["masks"].shape) == (len(SIZES), len(names), G, G)
    ref = reference_masks()
    for si in range(len(SIZES)):                                                                                 # the shapes do what their names say
        assert np.array_equal(ref[si, "two_vertex_ring_and_triangle"], ref[si, "triangle"]) and not ref[si, "two_vertex_ring_alone"].any()
        assert np.array_equal(ref[si, "random_300_compressed"], ref[si, "random_300"])


def test_batch_layout_mixed_kinds_none_and_padding(cuda):
    from boosted_detr_amd import pipeline
    h0, w0, h1, w1 = 37, 53, 64, 65
    p0, r0, p1, r1 = polygon_cases(h0, w0), rle_cases(h0, w0), polygon_cases(h1, w1), rle_cases(h1, w1)
    segs = [[p0["star_200"], {"size": [h0, w0], "counts": r0["random_300_compressed"]}, None, p0["nested_rings"], {"size": [h0, w0], "counts": r0["all_ones"]},
             p0["triangle"], p0["bowtie"]],                                         # 7 annotations: two are cut off at M = 5
            [{"size": [h1, w1], "counts": r1["random_300"]}, None, p1["concave_L"]]]  # 3 annotations: two padding rows
    records = [{"height": h, "width": w, "bbox": [[0.1, 0.1, 0.2, 0.2]] * len(s), "category": [["x"]] * len(s), "segmentation": s}
               for (h, w), s in zip([(h0, w0), (h1, w1)], segs)]
    batch = pipeline.pad_annotations(records, max_objects=5, with_masks=True)
    assert batch["segments"]["kind"].tolist() == [[1, 2, 0, 1, 2], [2, 0, 1, 0, 0]] and batch["num_objects"].tolist() == [5, 3]
    place = np.asarray([(96, 96, 50, 77, 46, 19), (64, 80, 40, 43, 0, 37)], np.int32)      # one placement per image
    got = pipeline.mask_targets(batch, placement=place)
    torch.cuda.synchronize()
    gm, ga = got["masks"].cpu().numpy(), got["mask_area"].cpu().numpy()
    assert gm.shape == (2, 5, 23, 23) and ga.shape == (2, 5)
    for b, (h, w) in enumerate([(h0, w0), (h1, w1)]):
        for m in range(5):
            seg = segs[b][m] if m < len(segs[b]) else None
            want, area = R.target(R.segmentation_mask(seg, h, w), 23, tuple(place[b]))
            assert ga[b, m] == area and np.array_equal(gm[b, m].view(np.uint32), want.view(np.uint32)), (b, m)
            if seg is None:
                assert ga[b, m] == 0 and not gm[b, m].any()


def test_augmentations_move_the_masks_with_the_image(cuda):
    from boosted_detr_amd import pipeline
    from boosted_detr_amd import kernels as K
    from boosted_detr_amd.engine import to_device
    rng = np.random.default_rng(3)
    H, W, h, w = 96, 96, 37, 53
    segs = [[polygon_cases(h, w)["star_200"], {"size": [h, w], "counts": rle_cases(h, w)["random_300"]}], [polygon_cases(h, w)["bowtie"]]]
    records = [{"height": h, "width": w, "bbox": [[0.2, 0.3, 0.4, 0.5]] * len(s), "category": [["x"]] * len(s), "segmentation": s} for s in segs]
    batch = pipeline.pad_annotations(records, with_masks=True)
    batch["image"] = rng.random((2, H, W, 3)).astype(np.float32)
    params = {"rand_val": np.asarray([[96 / 50, 96 / 77], [1.0, 1.0]], np.float32), "new_h": np.asarray([50, 96], np.int32),
              "new_w": np.asarray([77, 96], np.int32), "off_h": np.asarray([46, 0], np.int32), "off_w": np.asarray([19, 0], np.int32),
              "contrast": np.asarray([1.1, 0.9], np.float32), "brightness": np.asarray([0.05, -0.05], np.float32),
              "saturation": np.asarray([1.0, 1.1], np.float32)}
    aug = pipeline.Augmentations(seed=0, jpeg_quality=False)
    out = aug.apply(batch, params)
    plain_batch = {k: v for k, v in batch.items() if k != "segments"}
    plain = aug.apply(plain_batch, params)
    torch.cuda.synchronize()
    assert set(out) == set(batch) | {"masks", "mask_area"} and set(plain) == set(plain_batch) and "masks" not in plain
    # the image and the boxes are what they were before masks existed: the kernel's own output and adjust_boxes
    ip = to_device(np.stack([params["new_h"], params["new_w"], params["off_h"], params["off_w"]], axis=-1).astype(np.int32), torch.int32)
    fp = to_device(np.stack([params["contrast"], params["brightness"], params["saturation"]], axis=-1).astype(np.float32))
    today = K.augment(to_device(batch["image"]), ip, fp, None)
    assert torch.equal(plain["image"], today) and torch.equal(out["image"], today)
    boxes = pipeline.Augmentations.adjust_boxes(batch["bbox"], params, H, W)
    assert np.array_equal(plain["bbox"], boxes) and np.array_equal(out["bbox"], boxes)
    gm, ga = out["masks"].cpu().numpy(), out["mask_area"].cpu().numpy()
    assert gm.shape == (2, 2, 23, 23)
    for b in range(2):
        pl = (H, W, int(params["new_h"][b]), int(params["new_w"][b]), int(params["off_h"][b]), int(params["off_w"][b]))
        for m in range(2):
            want, area = R.target(R.segmentation_mask(segs[b][m] if m < len(segs[b]) else None, h, w), 23, pl)
            assert ga[b, m] == area and np.array_equal(gm[b, m].view(np.uint32), want.view(np.uint32)), (b, m)
    assert not gm[0, :, :10].any() and gm[0].max() > 0            # image 0 sits in the canvas' lower part: rows above off_h = 46 stay empty


def test_train_step_and_evaluate_on_rasterised_targets(cuda):
    """configs[0]: one train step of DETR(train_panoptic_head=True) on masks from pad_annotations(with_masks=True) -> mask_targets
    logs the same Mask_Loss, bit for bit, as the same step (same seed, fresh model) fed the reference's float masks; evaluate runs."""
    from boosted_detr_amd import pipeline
    from boosted_detr_amd import kernels as K
    from boosted_detr_amd.training import SGD
    from oracle import detr_oracle as O
    from test_panoptic_train_gpu import _head_model
    cfg = O.CONFIG1
    host = O.make_batch(cfg, 2, 20, seed=1234, num_objects=[3, 7])
    h, w = 37, 53
    shapes, runs = polygon_cases(h, w), rle_cases(h, w)
    pool = [shapes["star_200"], {"size": [h, w], "counts": runs["random_300_compressed"]}, shapes["concave_L"], shapes["nested_rings"],
            {"size": [h, w], "counts": runs["run_over_three_columns"]}, shapes["triangle"], shapes["bowtie"]]
    n = [int(v) for v in np.asarray(host["num_objects"]).reshape(-1)]
    records = [{"height": h, "width": w, "bbox": np.asarray(host["bbox"])[b, :n[b]].tolist(), "category": [["x"]] * n[b], "segmentation": pool[:n[b]]}
               for b in range(2)]
    pack = pipeline.pad_annotations(records, max_objects=20, with_masks=True)
    got = pipeline.mask_targets(pack)
    want = np.zeros((2, 20, 23, 23), np.float32)
    for b in range(2):
        for m in range(n[b]):
            want[b, m] = R.target(R.segmentation_mask(pool[m], h, w), 23)[0]
    prev = K.set_deterministic(True)
    try:
        logs, start = [], None
        for masks in (got["masks"], want):
            model = _head_model(cfg)                     # initialisers are seeded per variable name: a fresh model is the same model
            model.compile(optimizer=SGD(learning_rate=1e-3, momentum=.9, nesterov=True, clipnorm=.1))
            model.forward_backward(dict(host, masks=want))                      # build-by-first-call
            if start is None:
                start = model.get_weights_dict()
            model.set_weights_dict(start)
            logs.append(model.logs_to_host(model.train_step(dict(host, masks=masks))))
        res = model.evaluate([dict(host, masks=got["masks"])], iou_types=("bbox", "segm"))
    finally:
        K.set_deterministic(prev)
    print("Mask_Loss", logs[0]["Mask_Loss"], logs[1]["Mask_Loss"], "loss", logs[0]["loss"])
    assert np.isfinite(logs[0]["loss"]) and np.isfinite(logs[0]["Mask_Loss"]) and logs[0]["Mask_Loss"] > 0
    assert logs[0]["Mask_Loss"] == logs[1]["Mask_Loss"] and logs[0]["loss"] == logs[1]["loss"]
    assert "mask_AP" in res and "AP" in res and res["num_images"] == 2
