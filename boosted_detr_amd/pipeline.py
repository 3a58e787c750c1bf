"""Input step in front of the hot path.

Mirrors the parts of /root/reference/ModelComponents/pipeline.py that shape the model's input dict:
``Pipeline.data_generator``'s padding contract (131-186: '<PAD>' strings, -10 boxes, num_objects) and
``Augmentations`` (260-341).  The reference builds a tf.data graph; here batches are plain dicts and
the image work runs in csrc/augment.hip.  Image decoding, TFRecords and the dataset downloaders stay
out of scope.
"""
from __future__ import annotations

from typing import Dict, Iterable, Iterator, List, Optional, Sequence

import numpy as np
import torch

from . import kernels as K
from .engine import to_device
from .panoptic_neck import MASK_GRID          # the mask head's output grid (23)

PAD = "<PAD>"
BOX_PAD = -10.0


def coco_records(coco: dict, normalise: bool = True, with_eval_fields: bool = False, with_masks: bool = False) -> List[dict]:
    """COCO-format annotations (``images``, ``annotations``, ``categories``) -> one record per image:
    {'image_id', 'file_name', 'width', 'height', 'category': [[name], ...], 'bbox': [[x,y,w,h], ...]}
    with boxes divided by [W,H,W,H] (README.md:131-158: normalised COCO format) - the per-image
    grouping datasets.py:340-516 performs with pandas.  with_eval_fields: each record also carries 'iscrowd': [0 / 1, ...] and
    'area': [pixels, ...] (the annotation's own, else w * h of its box), which Model.evaluate(coco=True) reads.  with_masks: each
    record also carries 'segmentation': [...] aligned with 'bbox' - the annotation's own polygon list or RLE dict, untouched (source
    pixels, never normalised), or None where it has none; pad_annotations(with_masks=True) packs them."""
    names = {c["id"]: c["name"] for c in coco["categories"]}
    by_image: Dict[int, dict] = {}
    for im in coco["images"]:
        by_image[im["id"]] = {"image_id": im["id"], "file_name": im.get("file_name", ""), "width": im["width"], "height": im["height"],
                              "category": [], "attribute": [], "bbox": []}
        if with_eval_fields:
            by_image[im["id"]].update(iscrowd=[], area=[])
        if with_masks:
            by_image[im["id"]]["segmentation"] = []
    for a in coco["annotations"]:
        rec = by_image[a["image_id"]]
        w, h = float(rec["width"]), float(rec["height"])
        x, y, bw, bh = a["bbox"]
        rec["bbox"].append([x / w, y / h, bw / w, bh / h] if normalise else [x, y, bw, bh])
        rec["category"].append([names[a["category_id"]]])
        rec["attribute"].append([str(t) for t in a.get("attribute_names", [])] or [PAD])
        if with_eval_fields:
            rec["iscrowd"].append(int(a.get("iscrowd", 0)))
            rec["area"].append(float(a["area"]) if "area" in a else float(bw) * float(bh))
        if with_masks:
            rec["segmentation"].append(a.get("segmentation"))
    return list(by_image.values())


def decode_rle_counts(counts) -> np.ndarray:
    """The ``counts`` of a COCO RLE -> int64 run lengths (zeros first, alternating).  A list is taken as it is; a str / bytes is the
    public compressed form: every count is a sequence of characters c = ord(ch) - 48 whose low 5 bits are the value's next 5 bits
    (least significant group first), bit 0x20 says that more groups follow, bit 0x10 of the last group sign-extends the value, and
    from the fourth count on the value stored is the difference to the count two places earlier.  A negative count, a character
    outside the alphabet or a string that ends inside a count is a ValueError."""
    if isinstance(counts, (str, bytes)):
        try:
            data = counts.encode("ascii") if isinstance(counts, str) else bytes(counts)
        except UnicodeEncodeError as e:
            raise ValueError(f"decode_rle_counts: character {counts[e.start]!r} is outside the RLE alphabet") from None
        out: List[int] = []
        p, n = 0, len(data)
        while p < n:
            x, k, more = 0, 0, True
            while more:
                if p >= n:
                    raise ValueError("decode_rle_counts: the string ends inside a count")
                c = data[p] - 48
                if not 0 <= c < 64:
                    raise ValueError(f"decode_rle_counts: character {chr(data[p])!r} is outside the RLE alphabet")
                x |= (c & 0x1F) << (5 * k)
                more = bool(c & 0x20)
                p += 1
                k += 1
                if not more and (c & 0x10):
                    x |= -1 << (5 * k)
            if len(out) > 2:
                x += out[-2]
            out.append(x)
        arr = np.asarray(out, np.int64)
    else:
        arr = np.asarray(counts)
        if arr.size and not np.issubdtype(arr.dtype, np.integer):
            raise ValueError("decode_rle_counts: counts must be integers")
        arr = arr.astype(np.int64).reshape(-1)
    if (arr < 0).any():
        raise ValueError("decode_rle_counts: negative run length")
    return arr


def encode_rle_counts(counts) -> str:
    """The inverse of decode_rle_counts: run lengths -> the COCO compressed string."""
    c = [int(v) for v in counts]
    out = []
    for i, v in enumerate(c):
        x = v - (c[i - 2] if i > 2 else 0)
        more = True
        while more:
            g = x & 0x1F
            x >>= 5
            more = (x != -1) if (g & 0x10) else (x != 0)
            out.append(chr((g | (0x20 if more else 0)) + 48))
    return "".join(out)


def _segment_items(seg, h: int, w: int):
    """One COCO segmentation -> (kind, int32 items) in the layout of bdetr_mask_targets (include/bdetr.h, K18)."""
    if seg is None:
        return K.MASK_KIND_NONE, np.zeros(0, np.int32)
    if not (1 <= h <= K.MASK_MAX_DIM and 1 <= w <= K.MASK_MAX_DIM):
        raise ValueError(f"segmentation of a {h} x {w} image: height and width must be in [1, {K.MASK_MAX_DIM}]")
    if isinstance(seg, dict):
        if [int(v) for v in seg["size"]] != [h, w]:
            raise ValueError(f"RLE size {list(seg['size'])} differs from the image's height, width {[h, w]}")
        counts = decode_rle_counts(seg["counts"])
        if int(counts.sum()) != h * w:
            raise ValueError(f"RLE counts sum to {int(counts.sum())}, the image has {h * w} pixels")
        ends = np.cumsum(counts)
        runs = np.stack([ends[1::2] - counts[1::2], counts[1::2]], axis=-1)
        return K.MASK_KIND_RLE, runs[runs[:, 1] > 0].astype(np.int32).reshape(-1)
    rings = [seg] if (len(seg) and np.isscalar(seg[0])) else list(seg)      # a bare ring is taken as one ring
    verts, offs = [], [0]
    for ring in rings:
        v = np.asarray(ring, np.float64).reshape(-1)
        if v.size % 2:
            raise ValueError("a polygon ring is a flat [x0, y0, x1, y1, ...]: odd number of coordinates")
        q = np.rint(v * 256.0)                                               # 1/256 pixel, round half to even
        if not np.isfinite(q).all() or (np.abs(q) > K.MASK_MAX_COORD).any():
            raise ValueError("polygon coordinates must stay within +-2^23 / 256 pixels")
        verts.append(q.astype(np.int32))
        offs.append(offs[-1] + v.size // 2)
    return K.MASK_KIND_POLY, np.concatenate([np.asarray([len(rings)] + offs, np.int32)] + verts)


def pad_annotations(records: Sequence[dict], max_objects: Optional[int] = None, with_eval_fields: bool = False,
                    with_masks: bool = False, with_image_ids: bool = False) -> Dict[str, np.ndarray]:
    """pipeline.py:139-181: ragged per-image lists -> uniform arrays.  category [B,M,1] (pad '<PAD>'),
    attribute [B,M,Amax] (pad '<PAD>'), bbox [B,M,4] (pad -10), num_objects [B].  with_eval_fields: also iscrowd int32 [B,M]
    (pad 0), area f32 [B,M] in pixels (pad 0) and height / width int32 [B], from records of coco_records(with_eval_fields=True).
    with_masks: also 'segments', the host pack mask_targets() rasterises, from records of coco_records(with_masks=True) - a dict of
    int32 arrays in the layout of bdetr_mask_targets (include/bdetr.h, K18): items [T], item_off [B M + 1], kind [B,M] (0 none /
    1 polygon / 2 RLE), hw [B,M,2], with the same M and the same truncation as bbox.  Polygon vertices are snapped to 1/256 pixel
    here; RLE counts (list or compressed string) become (start, length) one-runs.  An RLE whose size differs from the record's
    height, width, counts that do not sum to h * w, and sizes beyond 4096 are a ValueError.
    with_image_ids: also image_id, a list [B] of the records' 'image_id' as they are (what Model.coco_results writes into every
    entry of a result file); a record without one is a ValueError."""
    B = len(records)
    n = [len(r.get("bbox", [])) for r in records]
    M = max_objects if max_objects is not None else max(max(n), 1)
    amax = max([len(a) for r in records for a in r.get("attribute", [])] + [1])
    category = np.full((B, M, 1), PAD, dtype=object)
    attribute = np.full((B, M, amax), PAD, dtype=object)
    bbox = np.full((B, M, 4), BOX_PAD, np.float32)
    for b, r in enumerate(records):
        for m in range(min(n[b], M)):
            category[b, m, 0] = r["category"][m][0]
            atts = r.get("attribute", [[PAD]] * n[b])[m]
            attribute[b, m, :len(atts)] = atts
            bbox[b, m] = r["bbox"][m]
    out = {"category": category, "attribute": attribute, "bbox": bbox, "num_objects": np.minimum(np.asarray(n, np.int32), M)}
    if with_eval_fields:
        iscrowd, area = np.zeros((B, M), np.int32), np.zeros((B, M), np.float32)
        for b, r in enumerate(records):
            k = min(n[b], M)
            iscrowd[b, :k], area[b, :k] = r["iscrowd"][:k], r["area"][:k]
        out.update(iscrowd=iscrowd, area=area, height=np.asarray([r["height"] for r in records], np.int32),
                   width=np.asarray([r["width"] for r in records], np.int32))
    if with_masks:
        kind, hw = np.zeros((B, M), np.int32), np.zeros((B, M, 2), np.int32)
        chunks, sizes = [], np.zeros(B * M, np.int64)
        for b, r in enumerate(records):
            if "segmentation" not in r or len(r["segmentation"]) != n[b]:
                raise ValueError("pad_annotations(with_masks=True) needs records with a 'segmentation' list aligned with 'bbox': "
                                 "make them with coco_records(..., with_masks=True)")
            h, w = int(r["height"]), int(r["width"])
            for m in range(min(n[b], M)):
                kind[b, m], it = _segment_items(r["segmentation"][m], h, w)
                hw[b, m] = (h, w)
                chunks.append(it)
                sizes[b * M + m] = it.size
        if int(sizes.sum()) > np.iinfo(np.int32).max:
            raise ValueError("segmentations of one batch exceed 2^31 items")
        out["segments"] = {"items": np.concatenate(chunks + [np.zeros(0, np.int32)]).astype(np.int32),
                           "item_off": np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), "kind": kind, "hw": hw}
    if with_image_ids:
        if any("image_id" not in r for r in records):
            raise ValueError("pad_annotations(with_image_ids=True) needs records with an 'image_id' (coco_records gives them)")
        out["image_id"] = [r["image_id"] for r in records]
    return out




def mask_targets(batch_or_pack: dict, grid: int = MASK_GRID, placement=None) -> Dict[str, torch.Tensor]:
    """The 'segments' pack of pad_annotations(with_masks=True) (or a batch that carries one) -> {'masks': f32 [B,M,grid,grid] in
    [0, 1], 'mask_area': int32 [B,M]} in HBM, rasterised by csrc/maskraster.hip: masks[b,m,i,j] is the exact share of grid cell
    (i,j) that object m's mask covers, mask_area its set pixels at source resolution (for RLE pycocotools' area exactly).

    placement: None (the image fills the canvas), one (H, W, new_h, new_w, off_h, off_w) for every image, or an int array [B,6]: the
    source stretched to new_h x new_w and put at (off_h, off_w) of an H x W canvas - what Augmentations does to the image.

    The rule is this project's own, stated in integers in include/bdetr.h: polygons are filled even-odd at pixel centres with
    vertices snapped to 1/256 pixel (left / top boundaries inclusive, right / bottom exclusive), rings are ORed.  pycocotools
    rasterises polygon BOUNDARY pixels by another rule (an upsampled scan conversion), so boundary pixels can differ from its
    masks; RLE decoding is exact."""
    pack = batch_or_pack["segments"] if "segments" in batch_or_pack else batch_or_pack
    B = pack["kind"].shape[0]
    if placement is None:
        placement = (1, 1, 1, 1, 0, 0)
    pl = np.asarray(placement)
    if not np.issubdtype(pl.dtype, np.integer):
        raise ValueError("mask_targets: placement must be integers (H, W, new_h, new_w, off_h, off_w)")
    if pl.size not in (6, 6 * B):
        raise ValueError(f"mask_targets: placement must be 6 integers or [B,6] with B={B}, got shape {pl.shape}")
    if pl.size and (int(pl.min()) < 0 or int(pl.max()) > K.MASK_MAX_DIM):       # before the cast: a value past 2^31 must not wrap into range
        raise ValueError(f"mask_targets: placement values must be in [0, {K.MASK_MAX_DIM}], got {int(pl.min())} .. {int(pl.max())}")
    pl = np.ascontiguousarray(np.broadcast_to(pl.reshape(-1, 6), (B, 6))).astype(np.int32)
    masks, area = K.mask_targets(pack["items"], pack["item_off"], pack["kind"], pack["hw"], pl, grid)
    return {"masks": masks, "mask_area": area}


class Augmentations:
    """pipeline.py:260-341 on the GPU.  ``apply_image_augmentations`` maps over an iterable of batch dicts
    exactly like the reference maps over a tf.data.Dataset (downsizer -> contrast -> brightness ->
    jpeg quality -> saturation); the per-image random draws come from a seeded NumPy generator (TF's
    stream is not reproducible) and can be injected for tests.  jpeg_quality=False leaves the JPEG
    round trip out (pipeline.py:319-325: quality uniform in [70, 100)).

    A batch that carries 'segments' (pad_annotations(with_masks=True)) also gets 'masks' and 'mask_area' (mask_targets), placed
    by the SAME draw that moved the image: (H, W, new_h, new_w, off_h, off_w).  The masks follow the image's true geometry - the
    source stretched to new_h x new_w at (off_h, off_w) - while the boxes keep the reference's quirky arithmetic (adjust_boxes).

    with_valid_region=True: the output also carries 'valid_region', int32 [B,4] on the host, rows (off_h, off_w, new_h, new_w) of that
    same draw - the picture's place on the canvas, which DETR.call / BoostedDETR.call turn into a key mask over the padding tokens
    (include/bdetr.h K35).  With the default False the output has the keys it always had."""

    image_key, bbox_key, segments_key = "image", "bbox", "segments"
    mask_grid = MASK_GRID

    valid_region_key = "valid_region"

    def __init__(self, seed: int = 0, jpeg_quality: bool = True, with_valid_region: bool = False):
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.jpeg_quality = jpeg_quality
        self.with_valid_region = bool(with_valid_region)

    def draw(self, B: int, H: int, W: int) -> Dict[str, np.ndarray]:
        # rand_val = max(1, truncated_normal(mean .5, std .7)): mostly 1 (no down-size), up to ~1.9
        tn = self.rng.standard_normal((B, 2))
        bad = np.abs(tn) > 2.0
        while bad.any():
            tn[bad] = self.rng.standard_normal(int(bad.sum()))
            bad = np.abs(tn) > 2.0
        rand_val = np.maximum(1.0, 0.5 + 0.7 * tn).astype(np.float32)
        new_h = (np.float32(H) / rand_val[:, 0]).astype(np.int32)
        new_w = (np.float32(W) / rand_val[:, 1]).astype(np.int32)
        off_h = self.rng.integers(0, H - new_h + 1).astype(np.int32)
        off_w = self.rng.integers(0, W - new_w + 1).astype(np.int32)
        return {"rand_val": rand_val, "new_h": new_h, "new_w": new_w, "off_h": off_h, "off_w": off_w,
                "contrast": self.rng.uniform(0.8, 1.2, B).astype(np.float32),
                "brightness": self.rng.uniform(-0.1, 0.1, B).astype(np.float32),
                "saturation": self.rng.uniform(0.8, 1.2, B).astype(np.float32),
                "jpeg_quality": self.rng.integers(70, 100, B).astype(np.int32)}

    @staticmethod
    def adjust_boxes(bbox: np.ndarray, p: Dict[str, np.ndarray], H: int, W: int) -> np.ndarray:
        """pipeline.py:302-313, quirks included: the COCO [x,y,w,h] box is divided by [r_h, r_w, r_h, r_w]
        and the normalised [off_h, off_w, off_h, off_w] is added to all four entries (also to w and h,
        and also to the -10 padding rows)."""
        rv = p["rand_val"]
        denom = np.stack([rv[:, 0], rv[:, 1], rv[:, 0], rv[:, 1]], axis=-1)[:, None, :]
        oh = (p["off_h"] / np.float64(H)).astype(np.float32)
        ow = (p["off_w"] / np.float64(W)).astype(np.float32)
        shift = np.stack([oh, ow, oh, ow], axis=-1)[:, None, :]
        return (bbox / denom + shift).astype(np.float32)

    def apply(self, batch: dict, params: Optional[Dict[str, np.ndarray]] = None) -> dict:
        image = batch[self.image_key]
        image = to_device(image if isinstance(image, torch.Tensor) else np.asarray(image, np.float32))
        B, H, W, _ = image.shape
        p = params if params is not None else self.draw(B, H, W)
        ip = to_device(np.stack([p["new_h"], p["new_w"], p["off_h"], p["off_w"]], axis=-1).astype(np.int32), torch.int32)
        fp = to_device(np.stack([p["contrast"], p["brightness"], p["saturation"]], axis=-1).astype(np.float32))
        out = dict(batch)
        q = to_device(np.asarray(p["jpeg_quality"], np.int32), torch.int32) if (self.jpeg_quality and "jpeg_quality" in p) else None
        out[self.image_key] = K.augment(image, ip, fp, q)
        if self.bbox_key in batch:
            out[self.bbox_key] = self.adjust_boxes(np.asarray(batch[self.bbox_key], np.float32), p, H, W)
        if self.segments_key in batch:
            place = np.stack([np.full(B, H), np.full(B, W), p["new_h"], p["new_w"], p["off_h"], p["off_w"]], axis=-1).astype(np.int32)
            out.update(mask_targets(batch[self.segments_key], self.mask_grid, place))
        if self.with_valid_region:
            out[self.valid_region_key] = np.stack([p["off_h"], p["off_w"], p["new_h"], p["new_w"]], axis=-1).astype(np.int32)
        return out

    def apply_image_augmentations(self, dataset: Iterable[dict]) -> Iterator[dict]:
        for batch in dataset:
            yield self.apply(batch)
