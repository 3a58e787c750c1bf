"""Per-batch time of Model.evaluate at the headline config (configs[1]: batch 16, 640 x 640, 6 + 6 layers, 100 queries, COCO
vocabulary) next to a forward-only predict_raw loop over the same device-resident batches.

Three loops per repetition, each closed by one device synchronisation:
  forward   predict_raw only
  update    predict_raw + target preparation + DetectionEvaluator.update (the two detmetric kernels; no host read)
  evaluate  Model.evaluate: the update loop + result() (one device-to-host copy, host accumulate)
If update() read anything back per batch, `update` would sit above `forward` by a synchronisation per batch; it should not.

With --segm: the same at configs[4] (batch 1, 800 x 1333, ResNet-101, 6 + 6 layers, 300 queries, the panoptic head; M = 100 padded
objects with 23 x 23 mask targets) and two more loops:
  head           predict_raw + panoptic_masks(): the forward pass with the mask head's
  evaluate_segm  Model.evaluate(iou_types=("bbox", "segm")): per batch the head's forward and the kernels of csrc/maskmetric.hip
                 on top of `evaluate`, still one device-to-host copy
`evaluate` stays the box-only Model.evaluate.  --segm-model builds the same model and batches and runs the three box loops alone, so
the tool can be pointed at a package without iou_types (the commit before it) for the figure to compare with.

With --coco: the batches also carry iscrowd (a tenth of the objects), area, height and width, and one more loop per evaluate loop:
  evaluate_coco       Model.evaluate(coco=True): the kernels of K16 in place of K14's, six (range, max_det) accumulates on the host
  evaluate_segm_coco  (with --segm) Model.evaluate(coco=True, iou_types=("bbox", "segm")): K16 and K17
`evaluate` and `evaluate_segm` stay the short protocol on the same batches (they read none of the extra keys).

    python tools/eval_bench.py [--batches 8] [--reps 5] [--batch 16] [--image 640] [--layers 6] [--queries 100] [--segm | --segm-model] [--coco]
    rocprofv3 --kernel-trace --stats -d DIR -o eval -- python tools/eval_bench.py --reps 1     # det_* / mask_* rows: the kernels' own times
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_batch(B, H, W, M, C, seed, masks=False, coco=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    num_objects = np.clip(1 + rng.poisson(6.3, size=B), 1, M).astype(np.int32)
    category, attribute = np.zeros((B, M), np.int32), np.zeros((B, M, 3), np.int32)
    bbox = np.full((B, M, 4), -10.0, np.float32)
    for b in range(B):
        n = int(num_objects[b])
        category[b, :n] = rng.integers(2, C, size=n)
        bbox[b, :n, 0:2] = rng.uniform(0.0, 0.6, size=(n, 2))
        bbox[b, :n, 2:4] = rng.uniform(0.05, 0.4, size=(n, 2))
    host = {"image": rng.random((B, H, W, 3), dtype=np.float32), "category": category, "attribute": attribute, "bbox": bbox,
            "num_objects": num_objects}
    if masks:
        host["masks"] = (rng.random((B, M, 23, 23)) > 0.6).astype(np.float32)
    if coco:
        host["iscrowd"] = (rng.random((B, M)) < 0.1).astype(np.int32)
        host["area"] = (np.maximum(bbox[..., 2], 0) * np.maximum(bbox[..., 3], 0) * np.float32(0.7 * H * W)).astype(np.float32)
        host["height"], host["width"] = np.full(B, H, np.int32), np.full(B, W, np.int32)
    return {k: torch.from_numpy(v).cuda() for k, v in host.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--image", type=int, default=640)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--segm", action="store_true", help="configs[4] with the panoptic head; adds the head and evaluate_segm loops")
    ap.add_argument("--segm-model", action="store_true", help="the model and batches of --segm, the box-only loops alone")
    ap.add_argument("--coco", action="store_true", help="adds the evaluate_coco (and with --segm evaluate_segm_coco) loops: the full COCO protocol")
    args = ap.parse_args()
    head = args.segm or args.segm_model
    if head:
        args.batch, args.queries, H, W, extra = 1, 300, 800, 1333, {"backbone_name": "ResNet101", "with_panoptic_head": True}
    else:
        H, W, extra = args.image, args.image, {}
    from boosted_detr_amd import parameters
    from boosted_detr_amd.evaluation import DetectionEvaluator
    from boosted_detr_amd.model import DETR, _prepare_targets
    model = DETR(num_object_preds=args.queries, image_size=(H, W), num_encoder_blocks=args.layers, num_encoder_heads=8,
                 encoder_dim=256, num_decoder_blocks=args.layers, num_decoder_heads=8, decoder_dim=256, num_panoptic_heads=1, panoptic_dim=32,
                 vocab_dict=parameters.COCO_VOCAB, attribute_weight=0.0, **extra)
    batches = [make_batch(args.batch, H, W, 100, model.num_categories, 1234 + i, masks=head, coco=args.coco) for i in range(args.batches)]
    ev = DetectionEvaluator(model.num_categories)

    def forward():
        for b in batches:
            model.predict_raw(b)

    def update():
        ev.reset()
        for b in batches:
            cat, _, box = model.predict_raw(b)
            ids, _, bbox, nobj = _prepare_targets(model, b)
            ev.update(cat, box, ids, bbox, nobj)

    def evaluate():
        model.evaluate(batches, evaluator=ev)

    def head_forward():
        for b in batches:
            model.predict_raw(b)
            model.panoptic_masks()

    segm = {}

    def evaluate_segm():
        segm.update(model.evaluate(batches, evaluator=ev, iou_types=("bbox", "segm")))

    coco = {}

    def evaluate_coco():
        coco.update(model.evaluate(batches, coco=True))

    def evaluate_segm_coco():
        coco.update(model.evaluate(batches, coco=True, iou_types=("bbox", "segm")))

    loops = {"forward": forward, "update": update, "evaluate": evaluate}
    if args.coco:
        loops.update(evaluate_coco=evaluate_coco)
    if args.segm:
        loops.update(head=head_forward, evaluate_segm=evaluate_segm)
        if args.coco:
            loops.update(evaluate_segm_coco=evaluate_segm_coco)
    for fn in loops.values():            # build-by-first-call, allocator warm-up
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in loops}
    for _ in range(args.reps):
        for k, fn in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / args.batches)
    out = {"config": vars(args), "ms_per_batch": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "median_ms_per_batch": {k: round(float(np.median(v)), 3) for k, v in ms.items()},
           "spread_ms_per_batch": {k: round(float(max(v) - min(v)), 3) for k, v in ms.items()},
           "result": {k: v for k, v in ev.result().items() if k in ("AP", "AR", "num_detections", "num_ground_truths", "num_images")}}
    if args.segm:
        out["result"].update({k: segm[k] for k in ("mask_AP", "mask_AR")})
    if args.coco:
        out["coco_stats"] = {k: [round(float(v), 6) for v in coco[k]] for k in ("stats", "mask_stats") if k in coco}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
