"""COCO-style box and mask average precision for DETR / BoostedDETR.

The reference trains and never evaluates; this is the missing half of the Keras surface (``Model.evaluate``).  The per-image work -
turning queries into detections, ranking them, matching them to the ground truths at every IoU threshold - runs on the GPU
(csrc/detmetric.hip, include/bdetr.h K14; for masks csrc/maskmetric.hip, K15) and leaves a few bytes per detection in HBM;
``DetectionEvaluator.update`` and ``MaskEvaluator.update`` read nothing back.  ``result`` copies what was kept to the host once and
runs COCOeval's ``accumulate`` there in NumPy fp64; ``results`` does so for several evaluators with one copy between them.

``DetectionEvaluator`` / ``MaskEvaluator`` are the short form: no crowd regions (``iscrowd``), no area ranges (everything is "all"),
one ``max_dets``.  ``CocoEvaluator`` / ``CocoMaskEvaluator`` are the full protocol (K16 / K17): crowd regions are *ignore*, every
area range is matched on its own (a ground truth outside the range is *ignore*), and the accumulate runs per (range, max_det) -
the 12 numbers of pycocotools' ``summarize``.  ``CocoMaskEvaluator`` compares masks (``iouType="segm"``) on the panoptic head's own
23 x 23 output grid, prediction logits cut at 0 and [0,1] targets at 0.5 (a mask's area is its share of the grid times the image's
H x W).  ``CocoImageMaskEvaluator`` (K19-K22) compares them at image resolution instead: logits upsampled to the image and cut at 0,
ground truths as their exact source bitmasks, areas in pixels.  What remains different from pycocotools there: the polygon
boundary rule of K18 (boundary pixels can differ from pycocotools' scan conversion; RLE is exact) and an upsample rule that is this
project's own (bilinear in fp64, reproducible bit for bit; it agrees with torch's interpolate except within rounding of zero).  A
query's mask shares its box's class and score (DETR's convention).

``AttributeEvaluator`` / ``AttributeMaskEvaluator`` (K29-K31) score the third head: the full protocol with one more test for a true
positive, the F1 of the predicted attribute set against the ground truth's, averaged over a grid of IoU and F1 thresholds.

``PanopticEvaluator`` (K23-K26) is the COCO panoptic task's PQ / SQ / RQ at image resolution: the kept queries' upsampled logits merged
into one id per pixel, the ground truths made disjoint, panopticapi's matching in integers; ``accumulate_pq`` is its host half.

``CocoResults`` (K27 / K28) is the way out to the official tools: the entries of a COCO results file, every query's image-resolution
mask run-length encoded on the GPU so that only the runs reach the host.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

KEEP_BIT = 0x8000
MAX_THRESHOLDS = 15
RECALL_POINTS = np.linspace(0.0, 1.0, 101)
_BIT_OF_THRESHOLD = np.arange(MAX_THRESHOLDS)[:, None]
_EPS = np.spacing(1.0)


def precision_recall(scores, tp_bits, ig_bits, npig: int, T: int):
    """One class's curve, for both protocols: its detections (the caller has applied any rank cut) sorted by descending score with
    a stable sort, cumulative TP / FP at each of the T thresholds (bit t of tp_bits; a detection whose bit t of ig_bits is set is
    neither - ig_bits None: none is), the right-to-left envelope, the precision at the 101 recall points.  npig: the class's
    non-ignored ground truths, > 0.  Returns (precision [T,R], recall [T])."""
    rank = np.argsort(-scores.astype(np.float64), kind="stable")
    shifts = _BIT_OF_THRESHOLD[:T]
    tp = ((tp_bits[rank][None, :] >> shifts) & 1).astype(np.float64)             # [T, D]
    counted = tp if ig_bits is None else np.maximum(tp, ((ig_bits[rank][None, :] >> shifts) & 1).astype(np.float64))
    tp_sum, fp_sum = np.cumsum(tp, axis=1), np.cumsum(1.0 - counted, axis=1)    # fp = ~tp & ~ig
    nd = rank.size
    rc = tp_sum / float(npig)
    pr = tp_sum / (fp_sum + tp_sum + _EPS)
    pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]                     # the right-to-left monotone envelope
    precision = np.zeros((T, RECALL_POINTS.size))
    for t in range(T):
        at = np.searchsorted(rc[t], RECALL_POINTS, side="left")
        inside = at < nd
        row = precision[t]                                                       # (a 1-D boolean store: the fast path)
        row[inside] = pr[t, at[inside]]
    return precision, (rc[:, -1] if nd else np.zeros(T))


def accumulate(records: Sequence[tuple], gt_count, iou_thresholds) -> Dict[str, object]:
    """COCOeval.accumulate over what the matching kernel left.

    records: per batch, in arrival order, ``(score f32 [B,N], label i32 [B,N], tp_bits u16 [B,N], order i32 [B,N])`` host arrays;
    gt_count: ground truths per class [C]; iou_thresholds: the T thresholds the bits of ``tp_bits`` stand for.
    Per class the detections are lined up image by image, each image's in the kernel's ``order``, and sorted by descending
    score with a stable sort; a class without ground truth takes part in no mean."""
    thr = np.asarray(iou_thresholds, np.float64).reshape(-1)
    gt_count = np.asarray(gt_count, np.int64).reshape(-1)
    T, C = thr.size, gt_count.size
    scores, labels, bits = [], [], []
    for score, label, tp_bits, order in records:
        order = np.asarray(order, np.int64)
        ok = order >= 0
        idx = np.where(ok, order, 0)
        s = np.take_along_axis(np.asarray(score, np.float32), idx, 1)[ok]
        l = np.take_along_axis(np.asarray(label, np.int64), idx, 1)[ok]
        t = np.take_along_axis(np.asarray(tp_bits).astype(np.int64) & 0xFFFF, idx, 1)[ok]      # row-major: image by image, ranked
        kept = (t & KEEP_BIT) != 0
        scores.append(s[kept]); labels.append(l[kept]); bits.append(t[kept])
    scores = np.concatenate(scores) if scores else np.zeros(0, np.float32)
    labels = np.concatenate(labels) if labels else np.zeros(0, np.int64)
    bits = np.concatenate(bits) if bits else np.zeros(0, np.int64)

    precision = np.full((T, RECALL_POINTS.size, C), -1.0)
    recall = np.full((T, C), -1.0)
    for c in np.flatnonzero(gt_count > 0):
        sel = labels == c
        precision[:, :, c], recall[:, c] = precision_recall(scores[sel], bits[sel], None, gt_count[c], T)
    valid = gt_count > 0

    def mean_ap(rows) -> float:
        p = precision[rows][:, :, valid]
        return float(p.mean()) if p.size else float("nan")

    def at_threshold(value: float) -> float:
        hit = np.flatnonzero(np.isclose(thr, value, rtol=0.0, atol=1e-9))
        return mean_ap(hit[:1]) if hit.size else float("nan")

    per_class = np.full(C, np.nan)
    if T:
        per_class[valid] = precision[:, :, valid].mean(axis=(0, 1))
    r = recall[:, valid]
    return {"AP": mean_ap(np.arange(T)), "AP50": at_threshold(0.5), "AP75": at_threshold(0.75),
            "AR": float(r.mean()) if r.size else float("nan"),
            "per_class_AP": per_class, "num_detections": int(bits.size), "num_ground_truths": int(gt_count[valid].sum()),
            "num_images": int(sum(np.asarray(rec[0]).shape[0] for rec in records)), "gt_count": gt_count.copy()}


def _words(t):
    """A kept device tensor as flat int32 words: float32 by its bit pattern, int32 as it is, 16-bit integers widened."""
    import torch
    return (t.view(torch.int32) if t.dtype == torch.float32 else t.to(torch.int32)).reshape(-1)


def _from_words(words: np.ndarray, t) -> np.ndarray:
    """The host copy of _words(t) in t's shape: float32 by the bit pattern, int32 as it is, a 16-bit tensor as the uint16 pattern."""
    words = words.reshape(tuple(t.shape))
    if t.dtype.is_floating_point:
        return words.view(np.float32)
    return words if t.element_size() == 4 else (words & 0xFFFF).astype(np.uint16)


class _KeptRecords:
    """What every evaluator keeps and how it reaches the host.  ``_kept`` holds one record per batch, a tuple of device tensors
    (float32, int32 or 16-bit integers); ``_gt_shape()`` is the shape of the running ground-truth counts ``_gt_count`` that follow
    them (None: there are none).  ``result`` makes ONE device-to-host copy - every record field by field, then the counts, as
    int32 words in one torch.cat - and hands ``result_from`` the records as host arrays (and the counts as int64); ``results``
    does that for several evaluators with one copy between them."""

    def _gt_shape(self) -> Optional[tuple]:
        return None

    def _device_parts(self) -> list:
        parts = [_words(t) for rec in self._kept for t in rec]
        return parts if self._gt_shape() is None else parts + [self._gt_count.reshape(-1)]

    def _from_flat(self, flat: np.ndarray, o: int = 0):
        """The host copy of _device_parts(), concatenated, from word o on -> (result_from's arguments, the word after them)."""
        records = []
        for rec in self._kept:
            host = []
            for t in rec:
                host.append(_from_words(flat[o:o + t.numel()], t))
                o += t.numel()
            records.append(tuple(host))
        shape = self._gt_shape()
        if shape is None:
            return (records,), o
        n = int(np.prod(shape))
        return (records, flat[o:o + n].astype(np.int64).reshape(shape)), o + n

    def _nothing(self) -> tuple:
        """result_from's arguments of an evaluator that saw no batch."""
        shape = self._gt_shape()
        return ([],) if shape is None else ([], np.zeros(shape, np.int64))

    def _host_args(self) -> tuple:
        import torch
        if not self._kept:
            return self._nothing()
        return self._from_flat(torch.cat(self._device_parts()).cpu().numpy())[0]

    def result(self) -> Dict[str, object]:
        return self.result_from(*self._host_args())


def _check_classes(num_classes: int, cat_pred) -> None:
    if cat_pred.shape[-1] != num_classes:
        raise ValueError(f"cat_pred has {cat_pred.shape[-1]} classes, the evaluator was built for {num_classes}")


class DetectionEvaluator(_KeptRecords):
    """Running COCO-style box AP.  ``update`` launches bdetr_det_postprocess and bdetr_det_match on the current stream and keeps the
    per-batch score / label / tp_bits / order tensors and the running per-class ground-truth count in HBM; it reads nothing back.
    ``result`` makes one device-to-host copy and accumulates on the host (a few bytes per detection, once per evaluation)."""

    def __init__(self, num_classes: int, iou_thresholds=None, max_dets: int = 100):
        thr = np.linspace(0.5, 0.95, 10) if iou_thresholds is None else np.asarray(iou_thresholds, np.float64).reshape(-1)
        if not 1 <= thr.size <= MAX_THRESHOLDS:
            raise ValueError(f"1 to {MAX_THRESHOLDS} IoU thresholds, got {thr.size}")
        if num_classes < 3:
            raise ValueError("num_classes counts <PAD> and <OOV>: at least 3")
        if max_dets < 1:
            raise ValueError("max_dets must be positive")
        self.num_classes, self.iou_thresholds, self.max_dets = int(num_classes), thr.astype(np.float64), int(max_dets)
        self.reset()

    def reset(self) -> None:
        self._kept: List[tuple] = []          # per batch: (score, label, tp_bits, order) device tensors
        self._gt_count = None                 # int32 [C] in HBM, allocated by the first update
        self.last_matched_gt = None           # int32 [B,T,N] of the last batch (inspection / tests)

    def update(self, cat_pred, box_pred, cat_ids, bbox, num_objects) -> None:
        """cat_pred [B,N,C] probabilities and box_pred [B,N,4] from ``Model.predict_raw``; cat_ids int32 [B,M], bbox f32 [B,M,4]
        (normalised COCO [x,y,w,h], -10 padding) and num_objects int32 [B] as ``_prepare_targets`` returns them.  All in HBM."""
        from . import kernels as K
        _check_classes(self.num_classes, cat_pred)
        self._count_on(cat_pred.device)
        score, label = K.det_postprocess(cat_pred.contiguous())
        order, tp_bits, matched = K.det_match(score, label, box_pred.contiguous(), cat_ids.contiguous(), bbox.contiguous(),
                                              num_objects.reshape(-1).contiguous(), self.iou_thresholds, self.num_classes, self.max_dets,
                                              self._gt_count)
        self._kept.append((score, label, tp_bits, order))
        self.last_matched_gt = matched

    def _gt_shape(self) -> tuple:
        return (self.num_classes,)

    def _count_on(self, device) -> None:
        """The running ground-truth counts, int32 in HBM, allocated by the first update."""
        import torch
        if self._gt_count is None:
            self._gt_count = torch.zeros(*self._gt_shape(), dtype=torch.int32, device=device)

    def _to_host(self):
        """One device-to-host copy -> (records, gt_count)."""
        return self._host_args()

    def result_from(self, records: Sequence[tuple], gt_count) -> Dict[str, object]:
        """The host half alone: accumulate over records as the kernels leave them (see ``accumulate``)."""
        return accumulate(records, gt_count, self.iou_thresholds)


def grid_mask_operands(num_classes: int, cat_pred, mask_logits, cat_ids, masks):
    """The shape checks of a grid-mask update() (MaskEvaluator, CocoMaskEvaluator).  Returns (B, N, M, mask_logits [B,N,P],
    masks [B,M,P])."""
    _check_classes(num_classes, cat_pred)
    if cat_pred.dim() != 3 or mask_logits.dim() not in (3, 4) or masks.dim() not in (3, 4) or cat_ids.dim() != 2:
        raise ValueError("expected cat_pred [B,N,C], mask_logits [B,N,P], cat_ids [B,M], masks [B,M,P]")
    B, N = cat_pred.shape[:2]
    M = cat_ids.shape[1]
    mask_logits, masks = mask_logits.reshape(B, mask_logits.shape[1], -1), masks.reshape(masks.shape[0], masks.shape[1], -1)
    if tuple(mask_logits.shape[:2]) != (B, N) or tuple(masks.shape[:2]) != (B, M) or mask_logits.shape[2] != masks.shape[2]:
        raise ValueError(f"mask_logits {tuple(mask_logits.shape)} and masks {tuple(masks.shape)} do not fit cat_pred [B={B},N={N},C] and "
                         f"cat_ids [B,M={M}] with one pixel count")
    return B, N, M, mask_logits, masks


class MaskEvaluator(DetectionEvaluator):
    """Running COCO-style mask AP (iouType="segm") on the panoptic head's grid.  ``update`` launches bdetr_det_postprocess, two
    bdetr_mask_binarize (logits at 0, targets at 0.5) and bdetr_mask_match on the current stream; what it keeps, and ``result``, are
    DetectionEvaluator's: the same records, the same ``accumulate``.  It reads nothing back per batch."""

    LOGIT_THRESHOLD, TARGET_THRESHOLD = 0.0, 0.5

    def update(self, cat_pred, mask_logits, cat_ids, masks, num_objects) -> None:
        """cat_pred [B,N,C] probabilities from ``Model.predict_raw``; mask_logits f32 [B,N,P] (or [B,N,h,w]) from ``panoptic_masks``;
        cat_ids int32 [B,M]; masks f32 [B,M,P] (or [B,M,h,w]) targets in [0,1], row m belonging to cat_ids row m; num_objects
        int32 [B].  All in HBM."""
        from . import kernels as K
        B, N, M, mask_logits, masks = grid_mask_operands(self.num_classes, cat_pred, mask_logits, cat_ids, masks)
        self._count_on(cat_pred.device)
        score, label = K.det_postprocess(cat_pred.contiguous())
        det_bits, det_area = K.mask_binarize(mask_logits.contiguous(), self.LOGIT_THRESHOLD)
        gt_bits, gt_area = K.mask_binarize(masks.contiguous(), self.TARGET_THRESHOLD)
        order, tp_bits, matched = K.mask_match(score, label, det_bits, det_area, cat_ids.contiguous(), gt_bits, gt_area,
                                               num_objects.reshape(-1).contiguous(), self.iou_thresholds, self.num_classes, self.max_dets,
                                               self._gt_count)
        self._kept.append((score, label, tp_bits, order))
        self.last_matched_gt = matched


# ---------------------------------------------------------------------------------------------------------------------
# the full COCO protocol: crowd regions, area ranges, several max_dets (K16 / K17)
# ---------------------------------------------------------------------------------------------------------------------
MAX_AREA_RANGES = 4
COCO_AREA_RANGES = {"all": (0.0, 1e10), "small": (0.0, 32.0 ** 2), "medium": (32.0 ** 2, 96.0 ** 2), "large": (96.0 ** 2, 1e10)}


def _mean_valid(a: np.ndarray) -> float:
    """COCOeval.summarize's mean over the entries that exist (> -1), in C order; NaN (pycocotools: -1) when there is none."""
    a = a[a > -1]
    return float(np.mean(a)) if a.size else float("nan")


class _Lineup:
    """The kept detections of every record, image by image in the kernel's order: what every (range, max_det) accumulate starts from."""

    def __init__(self, records: Sequence[tuple], A: int):
        scores, labels, ranks, tps, igs = [], [], [], [], []
        for score, label, class_rank, tp_bits, ig_bits, order in records:
            order = np.asarray(order, np.int64)
            ok = order >= 0
            idx = np.where(ok, order, 0)
            tp = np.asarray(tp_bits).astype(np.int64) & 0xFFFF                                  # [A,B,N]
            ig = np.asarray(ig_bits).astype(np.int64) & 0xFFFF
            kept = ok & ((np.take_along_axis(tp[0], idx, 1) & KEEP_BIT) != 0)                   # row-major: image by image, ranked
            scores.append(np.take_along_axis(np.asarray(score, np.float32), idx, 1)[kept])
            labels.append(np.take_along_axis(np.asarray(label, np.int64), idx, 1)[kept])
            ranks.append(np.take_along_axis(np.asarray(class_rank, np.int64), idx, 1)[kept])
            tps.append(np.stack([np.take_along_axis(tp[a], idx, 1)[kept] for a in range(A)]))
            igs.append(np.stack([np.take_along_axis(ig[a], idx, 1)[kept] for a in range(A)]))
        self.scores = np.concatenate(scores) if scores else np.zeros(0, np.float32)
        self.labels = np.concatenate(labels) if labels else np.zeros(0, np.int64)
        self.ranks = np.concatenate(ranks) if ranks else np.zeros(0, np.int64)
        self.tp = np.concatenate(tps, axis=1) if tps else np.zeros((A, 0), np.int64)
        self.ig = np.concatenate(igs, axis=1) if igs else np.zeros((A, 0), np.int64)


def accumulate_pair(lineup: _Lineup, npig, T: int, a: int, max_det: int):
    """COCOeval.accumulate for one area range and one max_det.  npig: the range's non-ignored ground truths per class [C].
    Returns (precision [T,R,C], recall [T,C]); -1 for a class with npig = 0."""
    npig = np.asarray(npig, np.int64).reshape(-1)
    C = npig.size
    precision = np.full((T, RECALL_POINTS.size, C), -1.0)
    recall = np.full((T, C), -1.0)
    within = lineup.ranks < max_det
    for c in np.flatnonzero(npig > 0):
        sel = within & (lineup.labels == c)
        precision[:, :, c], recall[:, c] = precision_recall(lineup.scores[sel], lineup.tp[a][sel], lineup.ig[a][sel], npig[c], T)
    return precision, recall


def accumulate_coco(records: Sequence[tuple], gt_count, iou_thresholds, max_dets, area_names) -> Dict[str, object]:
    """COCOeval.accumulate + summarize over what the K16 / K17 kernels left.

    records: per batch, in arrival order, ``(score f32 [B,N], label i32 [B,N], class_rank i32 [B,N], tp_bits u16 [A,B,N], ig_bits u16
    [A,B,N], order i32 [B,N])`` host arrays; gt_count [A,C]: the non-ignored ground truths per range and class; max_dets ascending;
    area_names: the A ranges' names, the first one being the base range ("all").  Only the (range, max_det) pairs that summarize
    reads are accumulated: every max_det in the base range, the largest max_det in every other range."""
    thr = np.asarray(iou_thresholds, np.float64).reshape(-1)
    gt_count = np.asarray(gt_count, np.int64)
    A, C = gt_count.shape
    T, last = thr.size, max_dets[-1]
    lineup = _Lineup(records, A)
    base_p, base_r = accumulate_pair(lineup, gt_count[0], T, 0, last)

    def at_threshold(value: float) -> float:
        hit = np.flatnonzero(np.isclose(thr, value, rtol=0.0, atol=1e-9))
        return _mean_valid(base_p[hit[0]]) if hit.size else float("nan")

    res = {"AP": _mean_valid(base_p), "AP50": at_threshold(0.5), "AP75": at_threshold(0.75)}
    ranged = [accumulate_pair(lineup, gt_count[a], T, a, last) for a in range(1, A)]
    for name, (p, _) in zip(area_names[1:], ranged):
        res[f"AP_{name}"] = _mean_valid(p)
    for m in max_dets:
        res[f"AR_{m}"] = _mean_valid(base_r if m == last else accumulate_pair(lineup, gt_count[0], T, 0, m)[1])
    for name, (_, r) in zip(area_names[1:], ranged):
        res[f"AR_{name}"] = _mean_valid(r)
    res["stats"] = [res[k] for k in list(res)]
    valid = gt_count[0] > 0
    per_class = np.asarray([_mean_valid(base_p[:, :, c]) for c in range(C)])
    res.update(AR=res[f"AR_{last}"], per_class_AP=per_class, num_detections=int(lineup.scores.size),
               num_ground_truths=int(gt_count[0][valid].sum()), num_images=int(sum(np.asarray(rec[0]).shape[0] for rec in records)),
               gt_count=gt_count[0].copy(), gt_count_per_range=gt_count.copy())
    return res


def crowd_flags(iscrowd, B: int, M: int, device):
    """iscrowd [B,M] (non-zero = crowd region; host or device) -> uint8 [B,M] in HBM."""
    import torch
    return (torch.as_tensor(iscrowd).to(device) != 0).to(torch.uint8).reshape(B, M).contiguous()


class CocoEvaluator(DetectionEvaluator):
    """Running box AP by the full COCO protocol: the 12 numbers of pycocotools' summarize.  ``update`` launches
    bdetr_det_postprocess and bdetr_det_match_coco (K16) on the current stream and reads nothing back; per batch it keeps score /
    label / class_rank / order [B,N] and tp_bits / ig_bits [A,B,N] in HBM.  ``result`` makes one device-to-host copy.
    area_ranges: a dict name -> (lo, hi) in pixels, the first entry being the base range (or a sequence of pairs, named all / small /
    medium / large by position); max_dets: ascending, the last one is the per-class truncation."""

    def __init__(self, num_classes: int, iou_thresholds=None, max_dets=(1, 10, 100), area_ranges=None):
        md = sorted({int(m) for m in (max_dets if np.ndim(max_dets) else [max_dets])})
        if not md or md[0] < 1:
            raise ValueError("max_dets must be positive")
        ranges = COCO_AREA_RANGES if area_ranges is None else area_ranges
        if not isinstance(ranges, dict):
            ranges = list(ranges)
            if len(ranges) > MAX_AREA_RANGES:
                raise ValueError(f"1 to {MAX_AREA_RANGES} area ranges, got {len(ranges)}")
            ranges = dict(zip(list(COCO_AREA_RANGES)[:len(ranges)], ranges))
        if not 1 <= len(ranges) <= MAX_AREA_RANGES:
            raise ValueError(f"1 to {MAX_AREA_RANGES} area ranges, got {len(ranges)}")
        super().__init__(num_classes, iou_thresholds, md[-1])
        self.max_dets = tuple(md)
        self.area_names = [str(k) for k in ranges]
        self.area_ranges = np.asarray([[float(lo), float(hi)] for lo, hi in ranges.values()], np.float64).reshape(-1, 2)

    def reset(self) -> None:
        super().reset()
        self._ranges_dev = None               # float64 [A,2] in HBM, allocated by the first update

    def _gt_shape(self) -> tuple:
        return (len(self.area_names), self.num_classes)

    def _coco_operands(self, device, B: int, M: int, iscrowd, area, image_hw):
        """iscrowd -> uint8 [B,M] (None: no crowd), area -> f32 [B,M] or None, image_hw -> int32 [B,2] ((H, W): every image's), all in HBM."""
        import torch
        self._count_on(device)
        if self._ranges_dev is None:
            self._ranges_dev = torch.from_numpy(self.area_ranges).to(device)
        crowd = torch.zeros(B, M, dtype=torch.uint8, device=device) if iscrowd is None else crowd_flags(iscrowd, B, M, device)
        if area is not None:
            area = torch.as_tensor(area).to(device=device, dtype=torch.float32).reshape(B, M).contiguous()
        if image_hw is None:
            raise ValueError("image_hw is needed: the images' original (height, width), one pair or int32 [B,2]")
        hw = torch.as_tensor(image_hw).to(device=device, dtype=torch.int32)
        hw = (hw.reshape(1, 2).expand(B, 2) if hw.numel() == 2 else hw.reshape(B, 2)).contiguous()
        return crowd, area, hw

    def update(self, cat_pred, box_pred, cat_ids, bbox, num_objects, iscrowd=None, area=None, image_hw=None) -> None:
        """As DetectionEvaluator.update, plus iscrowd [B,M] (non-zero = crowd region; None: none), area f32 [B,M] in pixels of the
        original image (None: from the box) and image_hw, the original (height, width): one pair for every image or int32 [B,2]."""
        from . import kernels as K
        _check_classes(self.num_classes, cat_pred)
        B, M = cat_ids.shape
        crowd, area, hw = self._coco_operands(cat_pred.device, B, M, iscrowd, area, image_hw)
        score, label = K.det_postprocess(cat_pred.contiguous())
        order, class_rank, tp_bits, ig_bits, matched = K.det_match_coco(
            score, label, box_pred.contiguous(), cat_ids.contiguous(), bbox.contiguous(), crowd, area, num_objects.reshape(-1).contiguous(), hw,
            self._ranges_dev, self.iou_thresholds, self.num_classes, self.max_dets[-1], self._gt_count)
        self._kept.append((score, label, class_rank, tp_bits, ig_bits, order))
        self.last_matched_gt = matched

    def result_from(self, records: Sequence[tuple], gt_count) -> Dict[str, object]:
        return accumulate_coco(records, gt_count, self.iou_thresholds, self.max_dets, self.area_names)


class CocoMaskEvaluator(CocoEvaluator):
    """Running mask AP (iouType="segm") by the full COCO protocol on the panoptic head's grid: MaskEvaluator's kernels with
    bdetr_mask_match_coco (K17) in place of bdetr_mask_match; what it keeps, and ``result``, are CocoEvaluator's."""

    LOGIT_THRESHOLD, TARGET_THRESHOLD = MaskEvaluator.LOGIT_THRESHOLD, MaskEvaluator.TARGET_THRESHOLD

    def update(self, cat_pred, mask_logits, cat_ids, masks, num_objects, iscrowd=None, area=None, image_hw=None) -> None:
        """As MaskEvaluator.update, plus iscrowd / area / image_hw as CocoEvaluator.update takes them (area None: from the mask)."""
        from . import kernels as K
        B, N, M, mask_logits, masks = grid_mask_operands(self.num_classes, cat_pred, mask_logits, cat_ids, masks)
        crowd, area, hw = self._coco_operands(cat_pred.device, B, M, iscrowd, area, image_hw)
        score, label = K.det_postprocess(cat_pred.contiguous())
        det_bits, det_pop = K.mask_binarize(mask_logits.contiguous(), self.LOGIT_THRESHOLD)
        gt_bits, gt_pop = K.mask_binarize(masks.contiguous(), self.TARGET_THRESHOLD)
        order, class_rank, tp_bits, ig_bits, matched = K.mask_match_coco(
            score, label, det_bits, det_pop, cat_ids.contiguous(), gt_bits, gt_pop, crowd, area, num_objects.reshape(-1).contiguous(), hw,
            self._ranges_dev, self.iou_thresholds, int(mask_logits.shape[2]), self.num_classes, self.max_dets[-1], self._gt_count)
        self._kept.append((score, label, class_rank, tp_bits, ig_bits, order))
        self.last_matched_gt = matched


# ---------------------------------------------------------------------------------------------------------------------
# attribute-aware AP: the IoU test AND an F1 test on the attribute sets (K29-K31)
# ---------------------------------------------------------------------------------------------------------------------
MAX_F1_THRESHOLDS = 16


def accumulate_attr(records: Sequence[tuple], gt_count, iou_thresholds, f1_thresholds, max_dets, area_names) -> Dict[str, object]:
    """accumulate_coco over what the K30 / K31 kernels left: the same per-range, per-max_det accumulate, run once per F1 threshold.

    records: per batch, in arrival order, ``(score f32 [B,N], label i32 [B,N], class_rank i32 [B,N], tp_bits u16 [F,A,B,N], ig_bits u16
    [F,A,B,N], order i32 [B,N])`` host arrays; gt_count [A,C] (it does not depend on f).  Every mean is COCO's mean over the entries
    > -1 with f pooled into it: AP over all T x F, AP_IoU50 / AP_IoU75 over F at that IoU, AP_F1_50 / AP_F1_75 over T at that F1."""
    thr = np.asarray(iou_thresholds, np.float64).reshape(-1)
    f1 = np.asarray(f1_thresholds, np.float64).reshape(-1)
    gt_count = np.asarray(gt_count, np.int64)
    A, C = gt_count.shape
    T, F, last = thr.size, f1.size, max_dets[-1]
    lineups = [_Lineup([(s, l, cr, np.asarray(tp)[f], np.asarray(ig)[f], o) for s, l, cr, tp, ig, o in records], A) for f in range(F)]
    base = [accumulate_pair(lineups[f], gt_count[0], T, 0, last) for f in range(F)]
    base_p, base_r = np.stack([p for p, _ in base]), np.stack([r for _, r in base])            # [F,T,R,C], [F,T,C]

    def where(values, value: float):
        hit = np.flatnonzero(np.isclose(values, value, rtol=0.0, atol=1e-9))
        return int(hit[0]) if hit.size else None

    def at_iou(value: float) -> float:
        t = where(thr, value)
        return _mean_valid(base_p[:, t]) if t is not None else float("nan")

    def at_f1(value: float) -> float:
        f = where(f1, value)
        return _mean_valid(base_p[f]) if f is not None else float("nan")

    res = {"AP": _mean_valid(base_p), "AP_IoU50": at_iou(0.5), "AP_IoU75": at_iou(0.75), "AP_F1_50": at_f1(0.5), "AP_F1_75": at_f1(0.75)}
    ranged = [[accumulate_pair(lineups[f], gt_count[a], T, a, last) for f in range(F)] for a in range(1, A)]
    for name, per_f in zip(area_names[1:], ranged):
        res[f"AP_{name}"] = _mean_valid(np.stack([p for p, _ in per_f]))
    for m in max_dets:
        res[f"AR_{m}"] = _mean_valid(base_r if m == last else np.stack([accumulate_pair(lineups[f], gt_count[0], T, 0, m)[1] for f in range(F)]))
    for name, per_f in zip(area_names[1:], ranged):
        res[f"AR_{name}"] = _mean_valid(np.stack([r for _, r in per_f]))
    res["stats"] = [res[k] for k in list(res)]
    valid = gt_count[0] > 0
    res.update(AR=res[f"AR_{last}"], AP_table=[[_mean_valid(base_p[f, t]) for f in range(F)] for t in range(T)],
               per_class_AP=np.asarray([_mean_valid(base_p[:, :, :, c]) for c in range(C)]), num_detections=int(lineups[0].scores.size),
               num_ground_truths=int(gt_count[0][valid].sum()), num_images=int(sum(np.asarray(rec[0]).shape[0] for rec in records)),
               gt_count=gt_count[0].copy(), gt_count_per_range=gt_count.copy())
    return res


class AttributeEvaluator(CocoEvaluator):
    """Running attribute-aware box AP (Fashionpedia's AP_IoU+F1, in this project's own words - include/bdetr.h, K29-K31; not claimed
    to equal fashionpedia-api bit for bit): CocoEvaluator with one more test for a true positive, the F1 of the detection's predicted
    attribute set (probability >= 0.5, never <PAD> / <OOV>) against the ground truth's at each of F thresholds.  ``update`` launches
    bdetr_det_postprocess, two bdetr_attr_pack (K29) and bdetr_det_match_attr (K30) on the current stream and reads nothing back; per
    batch it keeps score / label / class_rank / order [B,N] and tp_bits / ig_bits [F,A,B,N] in HBM.  ``result`` makes one
    device-to-host copy (it joins ``results``) and runs CocoEvaluator's accumulate per F1 threshold (``accumulate_attr``).
    num_attributes counts <PAD> and <OOV>; both threshold grids default to 0.5:0.05:0.95; empty_f1: the F1 of two empty sets, 1.0
    (they agree: many objects carry no attribute) or 0.0."""

    def __init__(self, num_classes: int, num_attributes: int, iou_thresholds=None, f1_thresholds=None, empty_f1: float = 1.0,
                 max_dets=(1, 10, 100), area_ranges=None):
        from . import kernels as K
        super().__init__(num_classes, iou_thresholds, max_dets, area_ranges)
        f1 = np.linspace(0.5, 0.95, 10) if f1_thresholds is None else np.asarray(f1_thresholds, np.float64).reshape(-1)
        if not 1 <= f1.size <= MAX_F1_THRESHOLDS:
            raise ValueError(f"1 to {MAX_F1_THRESHOLDS} F1 thresholds, got {f1.size}")
        if float(empty_f1) not in (0.0, 1.0):
            raise ValueError(f"empty_f1 is the F1 of two empty attribute sets, 0.0 or 1.0, got {empty_f1}")
        self.attr_words = K.attr_words(num_attributes)          # a ValueError outside [3, 4096]
        self.num_attributes, self.f1_thresholds, self.empty_f1 = int(num_attributes), f1.astype(np.float64), float(empty_f1)

    def _check_attributes(self, what: str, N: int, M: int, attribute_pred, attribute_hot, mask_words=None) -> None:
        """Every refusal of the gate, before anything is launched."""
        from . import kernels as K
        for name, t, rows in (("attribute_pred", attribute_pred, N), ("attribute_hot", attribute_hot, M)):
            if t.dim() != 3 or t.shape[1] != rows or t.shape[2] != self.num_attributes:
                raise ValueError(f"{name} is {tuple(t.shape)}, expected [B,{rows},{self.num_attributes}]: the evaluator was built for "
                                 f"{self.num_attributes} attributes")
        K.check_attr_gate(what, N, M, self.attr_words, self.f1_thresholds, self.empty_f1, mask_words)

    def update(self, cat_pred, attribute_pred, box_pred, cat_ids, attribute_hot, bbox, num_objects, iscrowd=None, area=None, image_hw=None) -> None:
        """As CocoEvaluator.update, plus attribute_pred f32 [B,N,A] probabilities from ``Model.predict_raw`` and attribute_hot f32
        [B,M,A], the multi-hot targets ``_prepare_targets`` returns (row m belonging to cat_ids row m).  All in HBM."""
        from . import kernels as K
        _check_classes(self.num_classes, cat_pred)
        B, M = cat_ids.shape
        self._check_attributes("AttributeEvaluator.update", cat_pred.shape[1], M, attribute_pred, attribute_hot)
        crowd, area, hw = self._coco_operands(cat_pred.device, B, M, iscrowd, area, image_hw)
        score, label = K.det_postprocess(cat_pred.contiguous())
        det_attr, det_count = K.attr_pack(attribute_pred.contiguous())
        gt_attr, gt_attr_count = K.attr_pack(attribute_hot.contiguous())
        order, class_rank, tp_bits, ig_bits, matched = K.det_match_attr(
            score, label, box_pred.contiguous(), det_attr, det_count, cat_ids.contiguous(), bbox.contiguous(), gt_attr, gt_attr_count, crowd, area,
            num_objects.reshape(-1).contiguous(), hw, self._ranges_dev, self.iou_thresholds, self.f1_thresholds, self.empty_f1, self.num_classes,
            self.max_dets[-1], self._gt_count)
        self._kept.append((score, label, class_rank, tp_bits, ig_bits, order))
        self.last_matched_gt = matched

    def result_from(self, records: Sequence[tuple], gt_count) -> Dict[str, object]:
        return accumulate_attr(records, gt_count, self.iou_thresholds, self.f1_thresholds, self.max_dets, self.area_names)


class AttributeMaskEvaluator(AttributeEvaluator):
    """Running attribute-aware mask AP on the panoptic head's grid: CocoMaskEvaluator's kernels with bdetr_mask_match_attr (K31) in
    place of bdetr_mask_match_coco; what it keeps, and ``result``, are AttributeEvaluator's."""

    LOGIT_THRESHOLD, TARGET_THRESHOLD = MaskEvaluator.LOGIT_THRESHOLD, MaskEvaluator.TARGET_THRESHOLD

    def update(self, cat_pred, attribute_pred, mask_logits, cat_ids, attribute_hot, masks, num_objects, iscrowd=None, area=None, image_hw=None) -> None:
        """As CocoMaskEvaluator.update, plus attribute_pred / attribute_hot as AttributeEvaluator.update takes them."""
        from . import kernels as K
        B, N, M, mask_logits, masks = grid_mask_operands(self.num_classes, cat_pred, mask_logits, cat_ids, masks)
        P = int(mask_logits.shape[2])
        self._check_attributes("AttributeMaskEvaluator.update", N, M, attribute_pred, attribute_hot, mask_words=(P + 63) // 64)
        crowd, area, hw = self._coco_operands(cat_pred.device, B, M, iscrowd, area, image_hw)
        score, label = K.det_postprocess(cat_pred.contiguous())
        det_bits, det_pop = K.mask_binarize(mask_logits.contiguous(), self.LOGIT_THRESHOLD)
        gt_bits, gt_pop = K.mask_binarize(masks.contiguous(), self.TARGET_THRESHOLD)
        det_attr, det_count = K.attr_pack(attribute_pred.contiguous())
        gt_attr, gt_attr_count = K.attr_pack(attribute_hot.contiguous())
        order, class_rank, tp_bits, ig_bits, matched = K.mask_match_attr(
            score, label, det_bits, det_pop, det_attr, det_count, cat_ids.contiguous(), gt_bits, gt_pop, gt_attr, gt_attr_count, crowd, area,
            num_objects.reshape(-1).contiguous(), hw, self._ranges_dev, self.iou_thresholds, self.f1_thresholds, self.empty_f1, P,
            self.num_classes, self.max_dets[-1], self._gt_count)
        self._kept.append((score, label, class_rank, tp_bits, ig_bits, order))
        self.last_matched_gt = matched


# ---------------------------------------------------------------------------------------------------------------------
# masks at image resolution (K19-K22)
# ---------------------------------------------------------------------------------------------------------------------
def host_image_hw(height, width) -> np.ndarray:
    """height / width [B] as HOST arrays or sequences (what pad_annotations(with_eval_fields=True) gives) -> int32 [B,2].  Device
    tensors are refused: the buffer sizes of the image-resolution path come from these values, and reading them back would be a
    host synchronisation per batch."""
    if height is None or width is None:
        raise ValueError("image-resolution masks need the batch's 'height' and 'width' (pad_annotations(with_eval_fields=True))")
    parts = []
    for name, v in (("height", height), ("width", width)):
        if hasattr(v, "is_cuda"):                                # a torch tensor
            if v.is_cuda:
                raise ValueError(f"image-resolution masks need '{name}' as a host array or sequence, not a device tensor: the buffer "
                                 "sizes come from it and nothing is read back per batch")
            v = v.numpy()
        a = np.asarray(v)
        if a.size == 0 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"image-resolution masks need '{name}' as integers [B], got {a.dtype} {a.shape}")
        parts.append(a.reshape(-1).astype(np.int64))
    if parts[0].size != parts[1].size:
        raise ValueError("'height' and 'width' must have one entry per image each")
    return np.stack(parts, axis=1).astype(np.int32)


def check_max_mask_bytes(max_mask_bytes: Optional[int]) -> int:
    """An evaluator's max_mask_bytes argument (None: CocoImageMaskEvaluator.DEFAULT_MAX_MASK_BYTES) -> the budget in bytes."""
    max_mask_bytes = CocoImageMaskEvaluator.DEFAULT_MAX_MASK_BYTES if max_mask_bytes is None else int(max_mask_bytes)
    if max_mask_bytes < 1:
        raise ValueError("max_mask_bytes must be positive")
    return max_mask_bytes


def check_image_mask_batch(segments, image_hw_host, N: int, max_mask_bytes: int):
    """Every refusal of an image-resolution update() that needs no device (CocoImageMaskEvaluator, PanopticEvaluator): the segments
    pack, the images' sizes, that every segmented object was annotated on its image's own (height, width), and the byte budget
    of the two bitmask buffers.  Returns (image_hw int32 [B,2], Hm, Wm)."""
    from . import kernels as K
    if not isinstance(segments, dict) or any(k not in segments for k in ("items", "item_off", "kind", "hw")):
        raise ValueError("image-resolution masks need the batch's 'segments': the host pack of pipeline.pad_annotations(..., "
                         "with_masks=True) (items, item_off, kind, hw); dense 'masks' are grid data")
    if hasattr(image_hw_host, "is_cuda"):
        if image_hw_host.is_cuda:
            raise ValueError("image_hw_host must be a host array [B,2], not a device tensor: the buffer sizes come from it")
        image_hw_host = image_hw_host.numpy()
    hw = np.asarray(image_hw_host)
    kind, seg_hw = segments["kind"], segments["hw"]
    if not isinstance(kind, np.ndarray) or kind.ndim != 2 or not isinstance(seg_hw, np.ndarray) or seg_hw.shape != kind.shape + (2,):
        raise ValueError("segments: kind must be a NumPy array [B,M] and hw [B,M,2]")
    B, M = kind.shape
    if hw.shape != (B, 2) or not np.issubdtype(hw.dtype, np.integer):
        raise ValueError(f"image_hw_host must be integers [B={B},2] (height, width), got {hw.dtype} {hw.shape}")
    hw = hw.astype(np.int32)
    Hm, Wm = K.mask_layout(hw)
    used = kind != K.MASK_KIND_NONE
    wrong = used & (seg_hw != hw[:, None, :]).any(axis=2)
    if wrong.any():
        b, m = (int(v[0]) for v in np.nonzero(wrong))
        raise ValueError(f"segments: object {m} of image {b} was annotated on a {tuple(int(v) for v in seg_hw[b, m])} image, the batch "
                         f"says (height, width) = {tuple(int(v) for v in hw[b])}")
    need = 8 * Hm * Wm * B * (int(N) + M)
    if need > max_mask_bytes:
        raise ValueError(f"the bitmask buffers of this batch need {need} bytes (8 Hm Wm B (N + M) with Hm={Hm}, Wm={Wm}, B={B}, N={N}, "
                         f"M={M}); max_mask_bytes is {max_mask_bytes}")
    return hw, Hm, Wm


def image_mask_operands(evaluator, cat_pred, mask_logits, cat_ids, segments, image_hw_host):
    """The checks of an image-resolution update() (CocoImageMaskEvaluator, PanopticEvaluator): the operands' shapes with the square
    grid G, then the evaluator's check_batch, then that the pack has cat_ids' rows.  Returns (B, N, M, G, image_hw int32 [B,2], Hm, Wm)."""
    _check_classes(evaluator.num_classes, cat_pred)
    if cat_pred.dim() != 3 or mask_logits.dim() not in (3, 4) or cat_ids.dim() != 2:
        raise ValueError("expected cat_pred [B,N,C], mask_logits [B,N,G,G], cat_ids [B,M]")
    B, N = cat_pred.shape[:2]
    M = cat_ids.shape[1]
    G = int(round(float(mask_logits.shape[2]) ** 0.5)) if mask_logits.dim() == 3 else int(mask_logits.shape[2])
    if tuple(mask_logits.shape[:2]) != (B, N) or mask_logits[0, 0].numel() != G * G:
        raise ValueError(f"mask_logits {tuple(mask_logits.shape)} do not fit cat_pred [B={B},N={N},C] with a square grid")
    hw, Hm, Wm = evaluator.check_batch(segments, image_hw_host, N)
    if segments["kind"].shape != (B, M):
        raise ValueError(f"segments: kind is {segments['kind'].shape}, cat_ids [B={B},M={M}]")
    return B, N, M, G, hw, Hm, Wm


class CocoImageMaskEvaluator(CocoEvaluator):
    """Running mask AP (iouType="segm") by the full COCO protocol AT IMAGE RESOLUTION, as a COCO user compares it: every query's
    logits are upsampled to its image's height x width and cut at 0 (bdetr_mask_upsample_bits, K19 - DETR's own segmentation
    post-processing), every ground truth is its exact source bitmask (bdetr_mask_source_bits, K20: polygons by K18's rule, RLE
    exactly), the two are intersected by popcount (bdetr_mask_inter, K21) and matched by COCOeval's rule
    (bdetr_mask_match_coco_inter, K22).  A mask's area is its pixel count.  What it keeps, and ``result``, are CocoEvaluator's; it
    reads nothing back per batch.

    max_mask_bytes: the budget for the two bitmask buffers of ONE batch, 8 Hm Wm B (N + M) bytes with Hm = max height and
    Wm = ceil(max width / 64); a batch over it is refused with a ValueError before anything is launched, and the evaluator stays
    usable.  The default is 1 GiB: sixteen 480 x 640 images with 100 queries and 100 ground-truth rows need 117 MiB, two
    1333 x 800 images 53 MiB."""

    DEFAULT_MAX_MASK_BYTES = 1 << 30

    def __init__(self, num_classes: int, iou_thresholds=None, max_dets=(1, 10, 100), area_ranges=None, max_mask_bytes: Optional[int] = None):
        super().__init__(num_classes, iou_thresholds, max_dets, area_ranges)
        self.max_mask_bytes = check_max_mask_bytes(max_mask_bytes)

    def check_batch(self, segments, image_hw_host, N: int):
        """Every refusal of update() that needs no device: the segments pack, the images' sizes, that every segmented object was
        annotated on its image's own (height, width), and the byte budget.  Returns (image_hw int32 [B,2], Hm, Wm)."""
        return check_image_mask_batch(segments, image_hw_host, N, self.max_mask_bytes)

    def update(self, cat_pred, mask_logits, cat_ids, segments, num_objects, image_hw_host, iscrowd=None, area=None) -> None:
        """cat_pred [B,N,C] and mask_logits f32 [B,N,G,G] (or [B,N,G*G]) in HBM as for CocoMaskEvaluator.update; cat_ids int32 [B,M];
        segments: the HOST pack of pad_annotations(with_masks=True), row m belonging to cat_ids row m; num_objects int32 [B];
        image_hw_host: HOST integers [B,2], every image's (height, width) - the size its segmentations were annotated on; iscrowd /
        area as CocoEvaluator.update takes them (area None: the mask's pixel count).  Every refusal comes before the first launch."""
        import torch
        from . import kernels as K
        B, N, M, G, hw, Hm, Wm = image_mask_operands(self, cat_pred, mask_logits, cat_ids, segments, image_hw_host)
        device = cat_pred.device
        # the ground truths first: mask_source_bits checks the whole pack on the host before it launches
        gt_bits, gt_pop = K.mask_source_bits(segments["items"], segments["item_off"], segments["kind"], segments["hw"], Hm, Wm, device=device)
        flat = torch.from_numpy(np.concatenate([hw.reshape(-1), hw[:, 0] * hw[:, 1]]).astype(np.int32)).to(device)      # one copy
        hw_dev, pix = flat[:2 * B].view(B, 2), flat[2 * B:]
        crowd, area, hw_dev = self._coco_operands(device, B, M, iscrowd, area, hw_dev)
        num_objects = num_objects.reshape(-1).contiguous()
        score, label = K.det_postprocess(cat_pred.contiguous())
        det_bits, det_pop = K.mask_upsample_bits(mask_logits.reshape(B, N, G, G).contiguous(), hw_dev, Hm, Wm)
        inter = K.mask_inter(det_bits, gt_bits, num_objects)
        order, class_rank, tp_bits, ig_bits, matched = K.mask_match_coco_inter(
            score, label, inter, det_pop, cat_ids.contiguous(), gt_pop, crowd, area, num_objects, hw_dev, pix, self._ranges_dev,
            self.iou_thresholds, self.num_classes, self.max_dets[-1], self._gt_count)
        self._kept.append((score, label, class_rank, tp_bits, ig_bits, order))
        self.last_matched_gt = matched


# ---------------------------------------------------------------------------------------------------------------------
# panoptic quality (K23-K26)
# ---------------------------------------------------------------------------------------------------------------------
def accumulate_pq(records: Sequence[tuple], num_classes: int, stuff_classes=()) -> Dict[str, object]:
    """panopticapi's PQStat over what bdetr_panoptic_match left.

    records: per batch, in arrival order, ``(gt_state [B,M], pred_state [B,N], match_inter [B,M], match_union [B,M], gt_label [B,M],
    pred_label [B,N])`` int32 host arrays.  Walked in (batch, image, row) order: a ground-truth row with state >= 0 is a TP of its
    class and adds (double)match_inter / (double)match_union to that class's running fp64 iou_sum, state -1 is a FN; a predicted
    row with state -1 is a FP of its class.  Per class PQ = iou_sum / (tp + fp / 2 + fn / 2), SQ = iou_sum / tp (0 without a TP),
    RQ = tp / (tp + fp / 2 + fn / 2); the averages are the means over the classes with tp + fp + fn > 0 - over all of them, over
    the things (every class not in stuff_classes) and over the stuff - and 0.0 with 0 classes when there is none."""
    C = int(num_classes)
    tp, fp, fn = np.zeros(C, np.int64), np.zeros(C, np.int64), np.zeros(C, np.int64)
    iou_sum = [0.0] * C
    images = 0
    for gt_state, pred_state, match_inter, match_union, gt_label, pred_label in records:
        gs, gl = np.asarray(gt_state, np.int64).reshape(-1), np.asarray(gt_label, np.int64).reshape(-1)
        ps, pl = np.asarray(pred_state, np.int64).reshape(-1), np.asarray(pred_label, np.int64).reshape(-1)
        mi, mu = np.asarray(match_inter, np.int64).reshape(-1), np.asarray(match_union, np.int64).reshape(-1)
        images += int(np.asarray(gt_state).shape[0])
        g_ok, p_ok = (gl >= 0) & (gl < C), (pl >= 0) & (pl < C)
        tp += np.bincount(gl[(gs >= 0) & g_ok], minlength=C)
        fn += np.bincount(gl[(gs == -1) & g_ok], minlength=C)
        fp += np.bincount(pl[(ps == -1) & p_ok], minlength=C)
        for k in np.flatnonzero((gs >= 0) & g_ok):                # row-major: image by image, row by row
            iou_sum[int(gl[k])] += float(mi[k]) / float(mu[k])
    pq, sq, rq = np.full(C, np.nan), np.full(C, np.nan), np.full(C, np.nan)
    scored = (tp + fp + fn) > 0
    for c in np.flatnonzero(scored):
        denom = float(tp[c]) + 0.5 * float(fp[c]) + 0.5 * float(fn[c])
        pq[c] = iou_sum[c] / denom
        sq[c] = iou_sum[c] / float(tp[c]) if tp[c] else 0.0
        rq[c] = float(tp[c]) / denom
    stuff = np.zeros(C, bool)
    stuff[[int(c) for c in stuff_classes]] = True

    def average(sel):
        pick = np.flatnonzero(scored & sel)
        if pick.size == 0:
            return 0.0, 0.0, 0.0, 0
        n = float(pick.size)
        return (sum(float(pq[c]) for c in pick) / n, sum(float(sq[c]) for c in pick) / n, sum(float(rq[c]) for c in pick) / n, int(pick.size))

    out: Dict[str, object] = {}
    for suffix, sel in (("", np.ones(C, bool)), ("_th", ~stuff), ("_st", stuff)):
        p, s, r, n = average(sel)
        out.update({"PQ" + suffix: p, "SQ" + suffix: s, "RQ" + suffix: r, "num_classes_scored" + suffix: n})
    out.update(per_class_PQ=pq, per_class_SQ=sq, per_class_RQ=rq, tp=tp, fp=fp, fn=fn, iou_sum=np.asarray(iou_sum, np.float64),
               num_images=images)
    return out


def check_min_area(min_area) -> int:
    if int(min_area) != min_area or int(min_area) < 0:
        raise ValueError(f"min_area must be a non-negative integer, got {min_area}")
    return int(min_area)


def stuff_flags(stuff_classes, num_classes: int, device):
    """The checked stuff class ids -> uint8 [C] in HBM, 1 for a stuff class; None when there is none."""
    import torch
    if not stuff_classes:
        return None
    flags = np.zeros(num_classes, np.uint8)
    flags[list(stuff_classes)] = 1
    return torch.from_numpy(flags).to(device)


class PanopticEvaluator(_KeptRecords):
    """Running panoptic quality (PQ / SQ / RQ of the COCO panoptic task) at image resolution.  ``update`` chains, on the current
    stream: the ground truths' exact source bitmasks (bdetr_mask_source_bits, K20) made exclusive in place
    (bdetr_panoptic_gt_exclusive, K25), bdetr_det_postprocess, the selection of the queries that become segments
    (bdetr_panoptic_select, K23: score > score_threshold, the kept queries of a stuff class merged), the per-pixel merge of their
    upsampled logits into pairwise disjoint masks (bdetr_panoptic_merge, K24), the popcount intersection of the two disjoint sets
    (bdetr_mask_inter, K21) and panopticapi's matching in integers (bdetr_panoptic_match, K26).  Per batch it keeps gt_state /
    match_inter / match_union / gt_label [B,M] and pred_state / pred_label [B,N] in HBM and reads nothing back; ``result`` makes one
    device-to-host copy and accumulates on the host (``accumulate_pq``).

    What differs from DETR's PostProcessPanoptic and panopticapi (include/bdetr.h, K24 / K26): a pixel that no kept query claims
    with a positive logit stays void; a predicted segment below min_area pixels is no segment (neither FP nor matchable) instead
    of being removed before a second argmax; the crowd rule sums over all crowd segments of the class.
    stuff_classes: class ids in [2, num_classes); max_mask_bytes: as CocoImageMaskEvaluator's."""

    DEFAULT_MAX_MASK_BYTES = CocoImageMaskEvaluator.DEFAULT_MAX_MASK_BYTES

    def __init__(self, num_classes: int, score_threshold: float = 0.85, min_area: int = 5, stuff_classes=(), max_mask_bytes: Optional[int] = None):
        if num_classes < 3:
            raise ValueError("num_classes counts <PAD> and <OOV>: at least 3")
        if not 0.0 <= float(score_threshold) < 1.0:
            raise ValueError(f"score_threshold must be in [0, 1), got {score_threshold}")
        self.num_classes, self.score_threshold, self.min_area = int(num_classes), float(score_threshold), check_min_area(min_area)
        self.stuff_classes = self.check_stuff_classes(stuff_classes, self.num_classes)
        self.max_mask_bytes = check_max_mask_bytes(max_mask_bytes)
        self.reset()

    @staticmethod
    def check_stuff_classes(stuff_classes, num_classes: int) -> tuple:
        """Sorted distinct class ids; anything that is not an integer in [2, num_classes) is a ValueError."""
        out = set()
        for c in ([] if stuff_classes is None else stuff_classes):
            if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)) or not 2 <= int(c) < num_classes:
                raise ValueError(f"stuff_classes must be class ids (integers) in [2, {num_classes}), got {c!r}")
            out.add(int(c))
        return tuple(sorted(out))

    def reset(self) -> None:
        self._kept: List[tuple] = []          # per batch: (gt_state, pred_state, match_inter, match_union, gt_label, pred_label)
        self._is_stuff = None                 # uint8 [C] in HBM, allocated by the first update that needs it
        self.last = None                      # the last batch's small intermediates, in HBM (inspection / tests)

    def check_batch(self, segments, image_hw_host, N: int):
        """CocoImageMaskEvaluator.check_batch's refusals and byte budget.  Returns (image_hw int32 [B,2], Hm, Wm)."""
        return check_image_mask_batch(segments, image_hw_host, N, self.max_mask_bytes)

    def update(self, cat_pred, mask_logits, cat_ids, segments, num_objects, image_hw_host, iscrowd=None) -> None:
        """cat_pred [B,N,C], mask_logits f32 [B,N,G,G] (or [B,N,G*G]), cat_ids int32 [B,M], num_objects int32 [B] in HBM; segments:
        the HOST pack of pad_annotations(with_masks=True); image_hw_host: HOST integers [B,2]; iscrowd [B,M] or None - exactly what
        CocoImageMaskEvaluator.update takes.  Every refusal comes before the first launch."""
        import torch
        from . import kernels as K
        B, N, M, G, hw, Hm, Wm = image_mask_operands(self, cat_pred, mask_logits, cat_ids, segments, image_hw_host)
        device = cat_pred.device
        gt_bits, _ = K.mask_source_bits(segments["items"], segments["item_off"], segments["kind"], segments["hw"], Hm, Wm, device=device)
        hw_dev = torch.from_numpy(hw).to(device)
        crowd = None if iscrowd is None else crowd_flags(iscrowd, B, M, device)
        if self._is_stuff is None:
            self._is_stuff = stuff_flags(self.stuff_classes, self.num_classes, device)
        num_objects = num_objects.reshape(-1).contiguous()
        gt_label = cat_ids.contiguous()
        gt_pop = K.panoptic_gt_exclusive(gt_bits, gt_label, num_objects, self.num_classes)
        score, label = K.det_postprocess(cat_pred.contiguous())
        seg_of = K.panoptic_select(score, label, self.score_threshold, self.num_classes, self._is_stuff)
        _, bits, pop = K.panoptic_merge(mask_logits.reshape(B, N, G, G).contiguous(), seg_of, hw_dev, Hm, Wm)
        inter = K.mask_inter(bits, gt_bits, num_objects)
        gt_state, pred_state, match_inter, match_union = K.panoptic_match(inter, pop, label, seg_of, gt_pop, gt_label, crowd, num_objects,
                                                                          self.num_classes, self.min_area)
        self._kept.append((gt_state, pred_state, match_inter, match_union, gt_label, label))
        self.last = {"seg_of": seg_of, "pred_pop": pop, "gt_pop": gt_pop, "inter": inter, "score": score}

    def _to_host(self) -> list:
        """One device-to-host copy -> the records."""
        return self._host_args()[0]

    def result_from(self, records: Sequence[tuple]) -> Dict[str, object]:
        """The host half alone: accumulate_pq over records as the kernels leave them (host int32 arrays; no device is needed)."""
        return accumulate_pq(records, self.num_classes, self.stuff_classes)


# ---------------------------------------------------------------------------------------------------------------------
# result files (K27 / K28)
# ---------------------------------------------------------------------------------------------------------------------
def category_id_table(vocabulary: Sequence[str], category_ids=None) -> List[int]:
    """The dataset's category id of every label: entry l - 2 belongs to label l >= 2, the vocabulary's entry l - 2.  category_ids:
    a dict name -> id or a COCO ``categories`` list of {"id", "name"}; None: the id is l - 2.  A vocabulary name the mapping lacks
    is a ValueError."""
    names = [str(n) for n in vocabulary]
    if category_ids is None:
        return list(range(len(names)))
    if isinstance(category_ids, dict):
        ids = dict(category_ids)
    else:
        try:
            ids = {c["name"]: c["id"] for c in category_ids}
        except (TypeError, KeyError):
            raise ValueError("category_ids must be a dict name -> id or a COCO 'categories' list of {'id', 'name'} entries") from None
    missing = [n for n in names if n not in ids]
    if missing:
        raise ValueError(f"category_ids has no id for {len(missing)} of the model's categories: {missing[:5]}")
    return [int(ids[n]) for n in names]


def batch_image_ids(batch: dict) -> list:
    """The batch's 'image_id' entry (pad_annotations(with_image_ids=True)) as a list of built-in values; a batch without one is a
    ValueError that names the key."""
    ids = batch.get("image_id")
    if ids is None:
        raise ValueError("a result file needs every batch's 'image_id', one per image (pipeline.pad_annotations(..., with_image_ids=True))")
    if hasattr(ids, "is_cuda"):
        ids = ids.cpu().numpy()
    ids = ids.tolist() if isinstance(ids, np.ndarray) else list(ids)
    return [v.item() if isinstance(v, np.generic) else v for v in ids]


class CocoResults:
    """The entries of a COCO results file, accumulated batch by batch: one per (image, query) in batch, image, query order,
        {"image_id", "category_id", "score", "bbox": [x, y, w, h] in pixels}
    and with masks also "segmentation": {"size": [h, w], "counts": ...}, the query's image-resolution mask as COCO's column-major
    RLE - what pycocotools' loadRes and the COCO servers take.  Everything is built-in Python types.

    ``update`` runs bdetr_det_postprocess and, with mask logits, bdetr_mask_upsample_bits (K19) and the run-length encoder
    (bdetr_mask_rle_count / bdetr_mask_rle_encode, K27 / K28) on the current stream: the bitmasks never leave HBM, only the run
    lengths do.  Per batch it reads the total of the counts back (to size their buffer) and makes ONE device-to-host copy of
    (counts, offset, scores, labels, boxes); the compressed strings are made on the host (pipeline.encode_rle_counts).
    ``update_from`` is the host half alone.

    vocabulary: the model's category names (label l >= 2 is entry l - 2); category_ids: see ``category_id_table``;
    score_threshold: only queries with score > (float32)score_threshold get an entry, and only their masks are encoded (None:
    every query); compress: counts as the compressed string (False: the list of ints); max_mask_bytes: the budget of one batch's
    bitmask buffer, 8 Hm Wm B N bytes, and of its run lengths - a batch over it is a ValueError before the launch that would need it."""

    def __init__(self, vocabulary: Sequence[str], category_ids=None, score_threshold: Optional[float] = None, compress: bool = True,
                 max_mask_bytes: Optional[int] = None):
        self.category_table = category_id_table(vocabulary, category_ids)
        if score_threshold is not None and not float(score_threshold) == float(score_threshold):
            raise ValueError("score_threshold must be a number or None")
        self.score_threshold = None if score_threshold is None else np.float32(score_threshold)
        self.compress = bool(compress)
        self.max_mask_bytes = check_max_mask_bytes(max_mask_bytes)
        self.reset()

    def reset(self) -> None:
        self._entries: List[dict] = []

    def check_batch(self, image_ids, image_hw_host, B: int, N: int, with_masks: bool):
        """Every refusal of update() that needs no device.  Returns (image_hw int32 [B,2], Hm, Wm); Hm = Wm = 0 without masks."""
        from . import kernels as K
        hw = np.asarray(image_hw_host)
        if hw.shape != (B, 2) or not np.issubdtype(hw.dtype, np.integer):
            raise ValueError(f"image_hw_host must be integers [B={B},2] (height, width), got {hw.dtype} {hw.shape}")
        if len(image_ids) != B:
            raise ValueError(f"'image_id' has {len(image_ids)} entries, the batch has {B} images")
        hw = hw.astype(np.int32)
        if not with_masks:
            return hw, 0, 0
        Hm, Wm = K.mask_layout(hw)
        need = 8 * Hm * Wm * B * int(N)
        if need > self.max_mask_bytes:
            raise ValueError(f"the bitmask buffer of this batch needs {need} bytes (8 Hm Wm B N with Hm={Hm}, Wm={Wm}, B={B}, N={N}); "
                             f"max_mask_bytes is {self.max_mask_bytes}")
        return hw, Hm, Wm

    def update(self, cat_pred, box_pred, image_ids, image_hw_host, mask_logits=None) -> None:
        """cat_pred [B,N,C] probabilities and box_pred [B,N,4] from ``Model.predict_raw``, in HBM; image_ids: B values; image_hw_host:
        HOST integers [B,2], every image's (height, width); mask_logits f32 [B,N,G,G] (or [B,N,G*G]) from ``panoptic_masks``, or None
        for entries without a segmentation.  Every refusal comes before the first launch."""
        import torch
        from . import kernels as K
        if cat_pred.dim() != 3 or tuple(box_pred.shape) != tuple(cat_pred.shape[:2]) + (4,):
            raise ValueError("expected cat_pred [B,N,C] and box_pred [B,N,4]")
        B, N = cat_pred.shape[:2]
        if cat_pred.shape[2] != len(self.category_table) + 2:
            raise ValueError(f"cat_pred has {cat_pred.shape[2]} classes, the vocabulary has {len(self.category_table)} + 2")
        if mask_logits is not None:
            if mask_logits.dim() not in (3, 4) or tuple(mask_logits.shape[:2]) != (B, N):
                raise ValueError(f"mask_logits {tuple(mask_logits.shape)} do not fit cat_pred [B={B},N={N},C]")
            G = int(round(float(mask_logits.shape[2]) ** 0.5)) if mask_logits.dim() == 3 else int(mask_logits.shape[2])
            if mask_logits[0, 0].numel() != G * G:
                raise ValueError(f"mask_logits {tuple(mask_logits.shape)} are no square grid")
        hw, Hm, Wm = self.check_batch(image_ids, image_hw_host, B, N, mask_logits is not None)
        score, label = K.det_postprocess(cat_pred.contiguous())
        parts = [score, label, box_pred.contiguous()]
        if mask_logits is not None:
            hw_dev = torch.from_numpy(hw).to(cat_pred.device)
            keep = None if self.score_threshold is None else (score > float(self.score_threshold)).to(torch.uint8)
            bits, _ = K.mask_upsample_bits(mask_logits.reshape(B, N, G, G).contiguous(), hw_dev, Hm, Wm)
            counts, offset = K.mask_rle_encode(bits, hw_dev, keep, max_bytes=self.max_mask_bytes)
            parts += [offset.view(torch.int32), counts]
        flat = torch.cat([_words(t) for t in parts]).cpu().numpy()          # the one copy
        o = 0
        host = []
        for t in parts:
            host.append(_from_words(flat[o:o + t.numel()], t))
            o += t.numel()
        if mask_logits is None:
            self.update_from(host[0], host[1], host[2], image_ids, hw)
        else:
            self.update_from(host[0], host[1], host[2], image_ids, hw, host[4], np.ascontiguousarray(host[3]).view(np.int64))

    def update_from(self, score, label, box, image_ids, image_hw, counts=None, offset=None) -> None:
        """The host half alone: score f32 [B,N], label int [B,N], box f32 [B,N,4] (normalised COCO [x,y,w,h]), image_ids [B], image_hw
        int [B,2] and, for masks, counts int32 [total] / offset int64 [B N + 1] as kernels.mask_rle_encode leaves them (a kept
        query's span must not be empty).  bbox is the box times [w, h, w, h], in Python floats from the fp32 values."""
        from .pipeline import encode_rle_counts
        score, label = np.asarray(score, np.float32), np.asarray(label, np.int64)
        box, hw = np.asarray(box, np.float32), np.asarray(image_hw, np.int64)
        B, N = score.shape
        if label.shape != (B, N) or box.shape != (B, N, 4) or hw.shape != (B, 2) or len(image_ids) != B:
            raise ValueError("expected score [B,N], label [B,N], box [B,N,4], image_ids [B] and image_hw [B,2]")
        if (counts is None) != (offset is None):
            raise ValueError("counts and offset come together")
        if offset is not None:
            counts, offset = np.asarray(counts), np.asarray(offset, np.int64).reshape(-1)
            if offset.shape != (B * N + 1,) or offset[0] != 0 or (np.diff(offset) < 0).any() or offset[-1] > counts.size:
                raise ValueError("offset must be the exclusive prefix sum [B N + 1] of the masks' run counts, inside counts")
        table = self.category_table
        if label.size and (int(label.min()) < 2 or int(label.max()) >= len(table) + 2):
            raise ValueError(f"labels must be in [2, {len(table) + 2}): <PAD> and <OOV> are no detection's class")
        kept = np.ones((B, N), bool) if self.score_threshold is None else score > self.score_threshold
        for b in range(B):
            image_id = image_ids[b].item() if isinstance(image_ids[b], np.generic) else image_ids[b]
            h, w = int(hw[b, 0]), int(hw[b, 1])
            scale = (float(w), float(h), float(w), float(h))
            for n in np.flatnonzero(kept[b]):
                entry = {"image_id": image_id, "category_id": table[int(label[b, n]) - 2], "score": float(score[b, n]),
                         "bbox": [float(box[b, n, k]) * scale[k] for k in range(4)]}
                if offset is not None:
                    runs = counts[offset[b * N + n]:offset[b * N + n + 1]]
                    if runs.size == 0:
                        raise ValueError(f"query {int(n)} of image {b} is kept but has no run lengths")
                    entry["segmentation"] = {"size": [h, w], "counts": encode_rle_counts(runs) if self.compress else [int(v) for v in runs]}
                self._entries.append(entry)

    def result(self) -> List[dict]:
        """The entries so far, in arrival order (a new list of the same dicts)."""
        return list(self._entries)

    def dump(self, path) -> None:
        """result() as JSON at `path`: a COCO results file."""
        import json
        with open(path, "w") as f:
            json.dump(self._entries, f)


def results(evaluators: Sequence[_KeptRecords]) -> List[Dict[str, object]]:
    """result() of several evaluators with ONE device-to-host copy between them: every evaluator's kept tensors in one torch.cat."""
    import torch
    live = [ev for ev in evaluators if ev._kept]
    flat = torch.cat([p for ev in live for p in ev._device_parts()]).cpu().numpy() if live else np.zeros(0, np.int32)
    out, o = [], 0
    for ev in evaluators:
        args, o = ev._from_flat(flat, o) if ev._kept else (ev._nothing(), o)
        out.append(ev.result_from(*args))
    return out
