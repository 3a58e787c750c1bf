"""Inference and evaluation of a training.Model: raw predictions, detections, segmentations and the panoptic merge, and the loops
of ``evaluate`` (box and mask AP, short and full COCO protocol), ``evaluate_panoptic`` (PQ), ``evaluate_attributes`` (AP with
the attribute F1 gate) and ``coco_results`` (the entries of a COCO results file) over the evaluators of evaluation.py.
``Inference`` is a stateless base class of training.Model: it defines no __init__ and adds no attribute; what it reads
(num_categories, num_object_preds, image_size, vocab_dict, _panoptic_inputs, panoptic_masks()) is the model's."""
from __future__ import annotations

import time
from typing import Dict, Iterable, List, Optional

import numpy as np
import torch

from . import evaluation
from . import kernels as K
from .engine import to_device


class Inference:
    def predict_raw(self, inputs: dict) -> List[torch.Tensor]:
        """[cat_preds [B,N,C], attribute_preds [B,N,A], box_preds [B,N,4]] of an inference-mode forward pass, left in HBM (call(training=
        False) decodes them to strings on the host).  Needs inputs["image"] only."""
        return self(inputs, training=False, raw=True)

    def detections(self, inputs: dict) -> Dict[str, torch.Tensor]:
        """Every query as a detection, in HBM: scores f32 [B,N] and labels int32 [B,N] (the most probable class among the vocabulary's,
        ids >= 2: never <PAD> or <OOV>), boxes f32 [B,N,4] normalised COCO [x,y,w,h]."""
        cat_preds, _, box_preds = self.predict_raw(inputs)
        scores, labels = K.det_postprocess(cat_preds.contiguous())
        return {"scores": scores, "labels": labels, "boxes": box_preds}

    def attribute_detections(self, inputs: dict) -> Dict[str, torch.Tensor]:
        """detections(inputs) plus every query's predicted attribute set, in HBM: attributes int64 [B,N,Wa], the attribute
        probabilities cut at >= 0.5 (the decode rule of InverseTokenization) and packed 64 to a word (bit a mod 64 of word a div 64;
        <PAD> and <OOV>, indices 0 and 1, are never set; include/bdetr.h, K29), and attribute_count int32 [B,N], their set bits."""
        cat_preds, attribute_preds, box_preds = self.predict_raw(inputs)
        scores, labels = K.det_postprocess(cat_preds.contiguous())
        bits, count = K.attr_pack(attribute_preds.contiguous())
        return {"scores": scores, "labels": labels, "boxes": box_preds, "attributes": bits, "attribute_count": count}

    IOU_TYPES = ("bbox", "segm")

    @classmethod
    def _check_iou_types(cls, iou_types) -> tuple:
        types = (iou_types,) if isinstance(iou_types, str) else tuple(iou_types)
        bad = [t for t in types if t not in cls.IOU_TYPES]
        if bad or not types:
            raise ValueError(f"iou_types must name one or both of {cls.IOU_TYPES}, got {iou_types!r}")
        return tuple(t for t in cls.IOU_TYPES if t in types)

    MASK_RESOLUTIONS = ("grid", "image")

    @classmethod
    def _check_mask_resolution(cls, mask_resolution, coco: bool) -> str:
        if mask_resolution not in cls.MASK_RESOLUTIONS:
            raise ValueError(f"mask_resolution must be one of {cls.MASK_RESOLUTIONS}, got {mask_resolution!r}")
        if mask_resolution == "image" and not coco:
            raise ValueError('mask_resolution="image" needs coco=True: the short protocol scores masks on the grid only')
        return mask_resolution

    @staticmethod
    def _image_mask_fields(batch: dict):
        """(segments, image_hw int32 [B,2] on the HOST) of a batch for the image-resolution path; a ValueError says what is missing."""
        segments = batch.get("segments")
        if segments is None:
            raise ValueError('mask_resolution="image" needs every batch\'s \'segments\', the host pack of pipeline.pad_annotations(..., '
                             "with_masks=True); dense 'masks' are grid data and are not enough")
        return segments, evaluation.host_image_hw(batch.get("height"), batch.get("width"))

    def _require_panoptic_head(self) -> None:
        """Raises unless the model can produce masks (DETR with a panoptic head overrides this)."""
        raise RuntimeError(f"{type(self).__name__} has no mask head: iou_types with 'segm' and segmentations() need a DETR built with "
                           "with_panoptic_head=True or train_panoptic_head=True")

    def segmentations(self, inputs: dict, resolution: str = "grid") -> Dict[str, torch.Tensor]:
        """detections(inputs) plus every query's mask, in HBM: mask_logits f32 [B,N,23,23] from the panoptic head and masks int64
        [B,N,W], the logits cut at 0 (sigmoid > 0.5) and packed 64 pixels to a word, row-major (bit p mod 64 of word p div 64;
        W = ceil(529/64) = 9).  Afterwards panoptic_masks() answers for this call.
        resolution="image": also image_masks int64 [B,N,Hm,Wm], the logits upsampled to each image's own height x width and cut at 0
        (include/bdetr.h, K19: Hm = max height, Wm = ceil(max width / 64), pixel (x, y) is bit x mod 64 of word [y, x div 64], zero
        outside the image), image_mask_area int32 [B,N], their pixel counts, and image_hw int32 [B,2].  It needs inputs["height"] and
        inputs["width"] as host arrays or sequences."""
        from .panoptic_neck import MASK_GRID
        if resolution not in self.MASK_RESOLUTIONS:
            raise ValueError(f"resolution must be one of {self.MASK_RESOLUTIONS}, got {resolution!r}")
        self._require_panoptic_head()
        if resolution == "image":
            hw = evaluation.host_image_hw(inputs.get("height"), inputs.get("width"))
            Hm, Wm = K.mask_layout(hw)
        out = self.detections(inputs)
        logits = self.panoptic_masks()
        B, N = logits.shape[:2]
        bits, _ = K.mask_binarize(logits.contiguous(), 0.0)
        out.update(mask_logits=logits.reshape(B, N, MASK_GRID, MASK_GRID), masks=bits)
        if resolution == "image":
            if hw.shape[0] != B:
                raise ValueError(f"'height' / 'width' have {hw.shape[0]} entries, the batch has {B} images")
            hw_dev = to_device(hw, torch.int32)
            image_bits, image_area = K.mask_upsample_bits(out["mask_logits"].contiguous(), hw_dev, Hm, Wm)
            out.update(image_masks=image_bits, image_mask_area=image_area, image_hw=hw_dev)
        return out

    def evaluate(self, x: Iterable[dict], steps: Optional[int] = None, evaluator=None, return_dict: bool = True, verbose: int = 0,
                 iou_types=("bbox",), mask_evaluator=None, coco: bool = False, mask_resolution: str = "grid"):
        """COCO-style AP over the batches of `x` (dicts as for training: strings or pre-tokenised ids).  Per batch: an inference-mode
        forward pass and the two kernels of csrc/detmetric.hip, nothing read back; one device-to-host copy at the end (evaluation.py).
        Changes nothing: weights, moving statistics, optimizer slots and counters, the step seed, captured steps and what
        panoptic_masks() answers for stay as they were.
        evaluator: a DetectionEvaluator (other thresholds / max_dets); it is reset first.  Returns its result() dict, or with
        return_dict=False the list [AP, AP50, AP75, AR].
        iou_types: "bbox" (box AP, the default), "segm" (mask AP on the panoptic head's 23 x 23 grid) or both.  "segm" needs a DETR
        with a panoptic head and inputs["masks"] in every batch (as train_panoptic_head does); per batch it adds the head's forward on
        that same call's features and the kernels of csrc/maskmetric.hip.  The dict gains mask_AP, mask_AP50, mask_AP75, mask_AR and
        per_class_mask_AP (with "segm" alone it holds those and the counts), the list the four mask numbers after the box ones;
        still one device-to-host copy.  mask_evaluator: a MaskEvaluator, as `evaluator` is for boxes.
        coco=True (or a passed CocoEvaluator / CocoMaskEvaluator): the full COCO protocol - crowd regions, area ranges, AR at several
        max_dets - through the kernels of K16 / K17 instead.  Optional batch keys: iscrowd [B,M] (non-zero: a crowd region, which is
        ignored rather than matched), area [B,M] in pixels of the original image, height / width [B] the original size; missing keys
        mean no crowd, the area of the box (or mask) and the model's image_size.  The dict gains AP_small, AP_medium, AP_large, AR_1,
        AR_10, AR_100, AR_small, AR_medium, AR_large and stats, the 12 numbers in pycocotools' summarize order (with "segm" the
        mask_ counterparts and mask_stats); return_dict=False returns stats, followed by mask_stats.
        mask_resolution: "grid" (the default: everything above) or "image", with coco=True only: "segm" is scored at image resolution,
        as a COCO user compares it - every query's logits upsampled to its image's height x width and cut at 0, every ground truth
        its exact source bitmask, areas in pixels (evaluation.CocoImageMaskEvaluator; csrc/maskimage.hip, K19-K22).  Every batch
        then needs 'segments' (pipeline.pad_annotations(with_masks=True); 'masks' are not read) and 'height' / 'width' as HOST arrays
        (with_eval_fields=True), each segmentation annotated on that size; a batch that lacks them, or whose bitmasks would exceed
        the evaluator's max_mask_bytes, is a ValueError before anything is launched for it.  Same keys in the result, still one
        device-to-host copy.  mask_evaluator: then a CocoImageMaskEvaluator."""
        from .model import _prepare_masks, _prepare_targets
        types = self._check_iou_types(iou_types)
        coco = bool(coco) or isinstance(evaluator, evaluation.CocoEvaluator) or isinstance(mask_evaluator, evaluation.CocoEvaluator)
        self._check_mask_resolution(mask_resolution, coco)
        image_masks = mask_resolution == "image" or isinstance(mask_evaluator, evaluation.CocoImageMaskEvaluator)      # its class selects the path
        box_ev = mask_ev = None
        if "bbox" in types:
            box_ev = self._fresh_evaluator(evaluator, evaluation.CocoEvaluator if coco else evaluation.DetectionEvaluator,
                                           "coco=True needs a CocoEvaluator as evaluator" if coco else None)
        if "segm" in types:
            self._require_panoptic_head()
            mask_class = evaluation.MaskEvaluator if not coco else evaluation.CocoImageMaskEvaluator if image_masks else evaluation.CocoMaskEvaluator
            refusal = f"coco=True needs a {mask_class.__name__} as mask_evaluator" + (' with mask_resolution="image"' if image_masks else "")
            mask_ev = self._fresh_evaluator(mask_evaluator, mask_class, refusal if coco else None)
        image_masks = image_masks and mask_ev is not None

        def per_batch(batch: dict) -> None:
            if image_masks:                               # every refusal of this batch before anything is launched for it
                segments, hw_host = self._image_mask_fields(batch)
                mask_ev.check_batch(segments, hw_host, self.num_object_preds)
            cat_ids, _, bbox, num_objects = _prepare_targets(self, batch)
            masks = _prepare_masks(batch, bbox.shape[0], bbox.shape[1]) if mask_ev is not None and not image_masks else None
            coco_fields = self._coco_fields(batch, bbox.shape[0], bbox.shape[1]) if coco else ()      # (iscrowd, area, image_hw)
            cat_preds, _, box_preds = self.predict_raw(batch)
            if box_ev is not None:
                box_ev.update(cat_preds, box_preds, cat_ids, bbox, num_objects, *coco_fields)
            if image_masks:
                mask_ev.update(cat_preds, self.panoptic_masks(), cat_ids, segments, num_objects, hw_host, *coco_fields[:2])
            elif mask_ev is not None:
                mask_ev.update(cat_preds, self.panoptic_masks(), cat_ids, masks, num_objects, *coco_fields)      # the head on this call's features

        def result() -> dict:
            parts = evaluation.results([ev for ev in (box_ev, mask_ev) if ev is not None])      # one copy for both
            counts = ("num_detections", "num_ground_truths", "num_images", "gt_count") + (("gt_count_per_range",) if coco else ())
            return parts[0] if mask_ev is None else self._with_mask_result(parts[0] if box_ev is not None else None, parts[-1], counts)

        prefixes = [p for p, ev in (("", box_ev), ("mask_", mask_ev)) if ev is not None]
        keys = [p + k for p in prefixes for k in ("AP", "AP50", "AP75", "AR")]
        res = self._evaluation_loop("evaluate", x, steps, per_batch, result, keys, verbose)
        if return_dict:
            return res
        return [v for p in prefixes for v in res[p + "stats"]] if coco else [res[k] for k in keys]

    def _fresh_evaluator(self, given, expected, refusal: Optional[str], *args):
        """`given`, or an `expected` built for this model's classes (and args); unless it is an `expected`, a ValueError(refusal)
        (refusal None: the short protocol takes what it is given); reset."""
        ev = given if given is not None else expected(self.num_categories, *args)
        if refusal is not None and not isinstance(ev, expected):
            raise ValueError(refusal)
        ev.reset()
        return ev

    @staticmethod
    def _with_mask_result(res: Optional[dict], mask_res: dict, counts: tuple) -> dict:
        """The box result (None: just the counts, which the two share) with the mask result's entries under mask_ names."""
        res = res if res is not None else {k: mask_res[k] for k in counts}
        res.update({f"mask_{k}": v for k, v in mask_res.items() if k not in counts and k != "per_class_AP"}, per_class_mask_AP=mask_res["per_class_AP"])
        return res

    def _evaluation_loop(self, name: str, x: Iterable[dict], steps: Optional[int], per_batch, result, keys, verbose: int) -> dict:
        """per_batch(batch) over at most `steps` batches of `x`, then result(); what panoptic_masks() answers for is put back
        whether a batch fails or not.  verbose: one line with the time, the steps and result()[k] for k in keys."""
        keep_panoptic = self._panoptic_inputs
        t0, n = time.time(), 0
        try:
            for step, batch in enumerate(x):
                if steps is not None and step >= steps:
                    break
                per_batch(batch)
                n += 1
        finally:
            self._panoptic_inputs = keep_panoptic      # panoptic_masks() keeps answering for the last call the user made
        res = result()
        if verbose:
            print(f"{name} - {time.time() - t0:.1f}s - {n} steps - " + " - ".join(f"{k}: {res[k]:.4f}" for k in keys))
        return res

    def _coco_fields(self, batch: dict, B: int, M: int):
        """(iscrowd, area, image_hw) of a batch for the COCO evaluators: the optional keys iscrowd / area [B,M] and height / width [B]."""

        def dev(v, dtype):
            return to_device(v if isinstance(v, torch.Tensor) else np.asarray(v), dtype)

        iscrowd = dev(batch["iscrowd"], torch.int32).reshape(B, M) if batch.get("iscrowd") is not None else None
        area = dev(batch["area"], torch.float32).reshape(B, M) if batch.get("area") is not None else None
        if (batch.get("height") is None) != (batch.get("width") is None):
            raise ValueError("a batch carries both of 'height' and 'width' or neither")
        if batch.get("height") is not None:
            hw = torch.stack([dev(batch["height"], torch.int32).reshape(B), dev(batch["width"], torch.int32).reshape(B)], 1).contiguous()
        else:
            hw = tuple(int(v) for v in self.image_size[:2])
        return iscrowd, area, hw

    def coco_results(self, x: Iterable[dict], steps: Optional[int] = None, iou_types=("bbox",), score_threshold: Optional[float] = None,
                     category_ids=None, compress: bool = True, path=None) -> List[dict]:
        """The entries of a COCO results file over the batches of `x` (the dicts evaluate() takes) - what pycocotools' loadRes and the
        COCO servers read (evaluation.CocoResults).  One entry per image and query, in batch, image, query order:
        {"image_id", "category_id", "score", "bbox": [x, y, w, h] in pixels}; with "segm" in iou_types also "segmentation":
        {"size": [h, w], "counts": str}, the query's mask at image resolution (segmentations(resolution="image")'s image_masks) as
        COCO's column-major RLE.  Built-in Python types throughout: json.dumps takes the list, and path= writes it.
        Every batch needs 'image_id', one per image (pipeline.pad_annotations(with_image_ids=True)); 'height' / 'width' give the
        pixel size of each image (absent: the model's image_size).  category_id: label l >= 2 is entry l - 2 of the model's category
        vocabulary, mapped through category_ids - a dict name -> id or a COCO 'categories' list; a name it lacks is a ValueError
        before the first batch - or l - 2 itself with None.  score_threshold: only the queries with score > threshold (as float32)
        get an entry, and only their masks are encoded.  compress=False: counts is the list of run lengths.
        "segm" needs the panoptic head and 'height' / 'width' as HOST arrays, and refuses otherwise before a launch.  Per batch it
        runs the forward pass, the head, K19 and the run-length encoder (csrc/maskrle.hip, K27 / K28): the bitmasks stay in HBM, the
        total of the run counts is read back to size their buffer, and one device-to-host copy brings (counts, offset, scores,
        labels, boxes); the compressed strings are made on the host.  "bbox" alone works on every model.
        Changes nothing, as evaluate(): weights, moving statistics, optimizer slots and counters, the step seed and what
        panoptic_masks() answers for stay as they were."""
        types = self._check_iou_types(iou_types)
        segm = "segm" in types
        if segm:
            self._require_panoptic_head()
        res = evaluation.CocoResults(self.vocab_dict["category"], category_ids, score_threshold, compress)

        def per_batch(batch: dict) -> None:
            image_ids = evaluation.batch_image_ids(batch)         # every refusal of this batch before anything is launched for it
            if segm or batch.get("height") is not None or batch.get("width") is not None:
                height, width = (v.cpu() if getattr(v, "is_cuda", False) and not segm else v for v in (batch.get("height"), batch.get("width")))
                hw = evaluation.host_image_hw(height, width)
            else:
                hw = np.tile(np.asarray([int(v) for v in self.image_size[:2]], np.int32), (len(image_ids), 1))
            res.check_batch(image_ids, hw, len(image_ids), self.num_object_preds, segm)
            cat_preds, _, box_preds = self.predict_raw(batch)
            res.update(cat_preds, box_preds, image_ids, hw, self.panoptic_masks() if segm else None)

        def result() -> dict:
            return {"entries": res.result()}

        entries = self._evaluation_loop("coco_results", x, steps, per_batch, result, (), 0)["entries"]
        if path is not None:
            res.dump(path)
        return entries

    def panoptic_segmentation(self, inputs: dict, score_threshold: float = 0.85, min_area: int = 5, stuff_classes=()) -> Dict[str, torch.Tensor]:
        """One id per pixel, in HBM: the queries with score > score_threshold become segments (the kept queries of a class in
        stuff_classes are one segment, the lowest of them), and per pixel the segment whose query has the largest positive
        upsampled logit wins (include/bdetr.h, K23 / K24).  Returns panoptic_ids int16 [B,Hm,64 Wm] (the segment's query index; -1:
        void, or outside the image; Hm = max height, Wm = ceil(max width / 64)), segment_label int32 [B,N] and segment_score f32
        [B,N] (every query's; a segment's are those of its query), segment_area int32 [B,N] (pixels; 0 where n is no segment or has
        fewer than min_area pixels - the pixels of such a segment are -1 in panoptic_ids) and image_hw int32 [B,2].  Needs the
        panoptic head and inputs["height"] / inputs["width"] as host arrays or sequences.  Afterwards panoptic_masks() answers for
        this call."""
        from .panoptic_neck import MASK_GRID
        self._require_panoptic_head()
        stuff = evaluation.PanopticEvaluator.check_stuff_classes(stuff_classes, self.num_categories)
        min_area = evaluation.check_min_area(min_area)
        hw = evaluation.host_image_hw(inputs.get("height"), inputs.get("width"))
        Hm, Wm = K.mask_layout(hw)
        cat_preds, _, _ = self.predict_raw(inputs)
        logits = self.panoptic_masks()
        B, N = logits.shape[:2]
        if hw.shape[0] != B:
            raise ValueError(f"'height' / 'width' have {hw.shape[0]} entries, the batch has {B} images")
        hw_dev = to_device(hw, torch.int32)
        is_stuff = evaluation.stuff_flags(stuff, self.num_categories, hw_dev.device)
        score, label = K.det_postprocess(cat_preds.contiguous())
        seg_of = K.panoptic_select(score, label, float(score_threshold), self.num_categories, is_stuff)
        ids, _, pop = K.panoptic_merge(logits.reshape(B, N, MASK_GRID, MASK_GRID).contiguous(), seg_of, hw_dev, Hm, Wm, with_bits=False)
        own = seg_of == torch.arange(N, device=seg_of.device, dtype=torch.int32)[None, :]
        is_segment = own & (pop >= max(min_area, 1))
        area = torch.where(is_segment, pop, torch.zeros_like(pop))
        # a small elementwise pass: the pixels of a segment below min_area become void
        flat = ids.reshape(B, -1)
        dropped = (flat >= 0) & ~torch.gather(is_segment, 1, flat.clamp(min=0).long())
        ids = torch.where(dropped, torch.full_like(flat, -1), flat).reshape(ids.shape)
        return {"panoptic_ids": ids, "segment_label": label, "segment_score": score, "segment_area": area, "image_hw": hw_dev}

    def evaluate_panoptic(self, x: Iterable[dict], steps: Optional[int] = None, evaluator=None, score_threshold: float = 0.85,
                          min_area: int = 5, stuff_classes=(), return_dict: bool = True, verbose: int = 0):
        """Panoptic quality (PQ / SQ / RQ of the COCO panoptic task) over the batches of `x`, at image resolution
        (evaluation.PanopticEvaluator; csrc/panopticmerge.hip, K23-K26).  Per batch: an inference-mode forward pass, the head on that
        call's features and the evaluator's kernels, nothing read back; one device-to-host copy at the end.  Changes nothing, as
        evaluate(): weights, moving statistics, optimizer slots and counters, the step seed and what panoptic_masks() answers for
        stay as they were.  Every batch needs what evaluate(coco=True, mask_resolution="image") needs: 'segments'
        (pipeline.pad_annotations(with_masks=True)), 'height' / 'width' as HOST arrays (with_eval_fields=True) and optionally
        'iscrowd'; a batch that lacks them, or whose bitmasks would exceed the evaluator's max_mask_bytes, is a ValueError before
        anything is launched for it.  evaluator: a PanopticEvaluator (it is reset first; its own threshold, min_area and stuff
        classes hold); otherwise one is built from score_threshold / min_area / stuff_classes.  Returns its result() dict, or with
        return_dict=False the list [PQ, SQ, RQ]."""
        from .model import _prepare_targets
        self._require_panoptic_head()
        ev = self._fresh_evaluator(evaluator, evaluation.PanopticEvaluator, "evaluate_panoptic needs a PanopticEvaluator as evaluator",
                                   score_threshold, min_area, stuff_classes)

        def per_batch(batch: dict) -> None:
            segments, hw_host = self._image_mask_fields(batch)      # every refusal of this batch before anything is launched for it
            ev.check_batch(segments, hw_host, self.num_object_preds)
            cat_ids, _, bbox, num_objects = _prepare_targets(self, batch)
            iscrowd, _, _ = self._coco_fields(batch, bbox.shape[0], bbox.shape[1])
            cat_preds, _, _ = self.predict_raw(batch)
            ev.update(cat_preds, self.panoptic_masks(), cat_ids, segments, num_objects, hw_host, iscrowd)

        keys = ("PQ", "SQ", "RQ")
        res = self._evaluation_loop("evaluate_panoptic", x, steps, per_batch, ev.result, keys, verbose)
        return res if return_dict else [res[k] for k in keys]

    def evaluate_attributes(self, x: Iterable[dict], steps: Optional[int] = None, iou_types=("bbox",), evaluator=None, mask_evaluator=None,
                            iou_thresholds=None, f1_thresholds=None, empty_f1: float = 1.0, return_dict: bool = True, verbose: int = 0):
        """Attribute-aware AP over the batches of `x` (the dicts evaluate(coco=True) takes; 'attribute' is in every batch): the full COCO
        protocol with one more test for a true positive - the F1 of the detection's predicted attribute set (probability >= 0.5)
        against the matched ground truth's must reach an F1 threshold - averaged over a grid of IoU and F1 thresholds
        (evaluation.AttributeEvaluator; csrc/attrmetric.hip, K29-K31).  The rule is modelled on Fashionpedia's AP_IoU+F1 and stated in
        this project's own words; it is not claimed to equal fashionpedia-api bit for bit.  Per batch: an inference-mode forward
        pass, bdetr_det_postprocess, two bdetr_attr_pack and the gated matcher, nothing read back; one device-to-host copy at the end.
        Changes nothing, as evaluate(): weights, moving statistics, optimizer slots and counters, the step seed and what
        panoptic_masks() answers for stay as they were.
        iou_types: "bbox" (every model), "segm" (masks on the panoptic head's 23 x 23 grid; needs the head and inputs["masks"]) or both;
        image-resolution masks with the gate are not built.  evaluator / mask_evaluator: an AttributeEvaluator / AttributeMaskEvaluator
        (reset first; its own thresholds hold); otherwise one is built from iou_thresholds / f1_thresholds (both default to
        0.5:0.05:0.95) and empty_f1, the F1 of two empty sets (1.0: they agree).  Returns the result() dict - AP (over all T x F),
        AP_IoU50, AP_IoU75, AP_F1_50, AP_F1_75, AP_small ... AR_large, stats (those fourteen), AP_table [T][F], per_class_AP and the
        counts; with "segm" the mask_ counterparts beside them - or with return_dict=False stats, followed by mask_stats."""
        from .model import _prepare_masks, _prepare_targets
        types = self._check_iou_types(iou_types)
        if "segm" in types:
            self._require_panoptic_head()
        args = (self.num_attributes, iou_thresholds, f1_thresholds, empty_f1)
        box_ev = mask_ev = None
        if "bbox" in types:
            box_ev = self._fresh_evaluator(evaluator, evaluation.AttributeEvaluator, "evaluate_attributes needs an AttributeEvaluator as evaluator", *args)
            if isinstance(box_ev, evaluation.AttributeMaskEvaluator):
                raise ValueError("evaluate_attributes needs an AttributeEvaluator as evaluator, not its mask form")
        if "segm" in types:
            mask_ev = self._fresh_evaluator(mask_evaluator, evaluation.AttributeMaskEvaluator,
                                            "evaluate_attributes needs an AttributeMaskEvaluator as mask_evaluator", *args)

        def per_batch(batch: dict) -> None:
            cat_ids, attribute_hot, bbox, num_objects = _prepare_targets(self, batch)
            masks = _prepare_masks(batch, bbox.shape[0], bbox.shape[1]) if mask_ev is not None else None
            coco_fields = self._coco_fields(batch, bbox.shape[0], bbox.shape[1])      # (iscrowd, area, image_hw)
            cat_preds, attribute_preds, box_preds = self.predict_raw(batch)
            if box_ev is not None:
                box_ev.update(cat_preds, attribute_preds, box_preds, cat_ids, attribute_hot, bbox, num_objects, *coco_fields)
            if mask_ev is not None:
                mask_ev.update(cat_preds, attribute_preds, self.panoptic_masks(), cat_ids, attribute_hot, masks, num_objects, *coco_fields)

        def result() -> dict:
            parts = evaluation.results([ev for ev in (box_ev, mask_ev) if ev is not None])      # one copy for both
            counts = ("num_detections", "num_ground_truths", "num_images", "gt_count", "gt_count_per_range")
            return parts[0] if mask_ev is None else self._with_mask_result(parts[0] if box_ev is not None else None, parts[-1], counts)

        prefixes = [p for p, ev in (("", box_ev), ("mask_", mask_ev)) if ev is not None]
        keys = [p + k for p in prefixes for k in ("AP", "AP_IoU50", "AP_F1_50", "AR")]
        res = self._evaluation_loop("evaluate_attributes", x, steps, per_batch, result, keys, verbose)
        return res if return_dict else [v for p in prefixes for v in res[p + "stats"]]
