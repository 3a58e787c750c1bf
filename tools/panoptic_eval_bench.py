"""Time of one batch of panoptic quality (K23-K26, csrc/panopticmerge.hip; evaluation.PanopticEvaluator) at the load of
tools/mask_image_eval_bench.py, next to mask AP at image resolution on the same batch:

  batch 16, 100 queries, 100 ground-truth rows, 480 x 640 images; per image 6 polygon objects of about 40 vertices and one crowd RLE
  of about 3,000 runs (tools/mask_targets_bench.py's generator), logits 3 N(0,1) on the 23 x 23 grid.

Two selections of the queries that become segments: "about 10" (the score threshold is the batch's 90th percentile of the scores)
and "all 100" (threshold 0).

What is timed (after warm-up; every window ends in a device synchronise; `reps` windows of `inner` calls, median and spread):
  K23 .. K26, K20, K21   each kernel alone on device-resident operands, between two device events; K24 with and without bits
  panoptic update        PanopticEvaluator.update: host checks, the copies, det_postprocess and the seven kernels; host clock
  K19, image update      bdetr_mask_upsample_bits and CocoImageMaskEvaluator.update on the same batch: the yardstick
For K24 the achieved bytes per second are set against its mandatory bytes, the bits and ids it writes: B Hm Wm (8 N + 128).
Nothing is read back inside a window.  K23 - K26 are compared with the plain-loop reference (tests/_panoptic_ref.py) on the first
image before anything is timed.

The report is printed and written to profiles/panoptic_eval_<date>.txt (or --out FILE): the committed profile IS this tool's output.

    python tools/panoptic_eval_bench.py [--reps 20] [--inner 20] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def fmt(r):
    return f"{r['median_ms']:10.4f} ms  ({r['min_ms']:.4f} - {r['max_ms']:.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None, help="where the report goes (default: profiles/panoptic_eval_<date>.txt)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU path: no GPU, no number"
    from mask_targets_bench import make_records, windows
    from boosted_detr_amd import evaluation, pipeline
    from boosted_detr_amd import kernels as K
    B, N, M, C, G, h, w, min_area = args.batch, 100, 100, 92, 23, 480, 640, 5
    records = make_records(B, h, w, polygons=6, vertices=40, runs=3000, seed=2024)
    rng = np.random.default_rng(7)
    for r in records:
        n = len(r["segmentation"])
        r.update(iscrowd=[0] * (n - 1) + [1], area=rng.uniform(200.0, 40000.0, n).tolist())
    batch = pipeline.pad_annotations(records, max_objects=M, with_eval_fields=True, with_masks=True)
    pack = batch["segments"]
    hw = evaluation.host_image_hw(batch["height"], batch["width"])
    Hm, Wm = K.mask_layout(hw)
    cat_pred = torch.softmax(torch.from_numpy(rng.standard_normal((B, N, C)).astype(np.float32)), -1).cuda()
    logits_host = (3.0 * rng.standard_normal((B, N, G, G))).astype(np.float32)
    logits = torch.from_numpy(logits_host).cuda()
    cat_ids_host = rng.integers(2, C, (B, M)).astype(np.int32)
    cat_ids = torch.from_numpy(cat_ids_host).cuda()
    num_objects = torch.from_numpy(batch["num_objects"].astype(np.int32)).cuda()
    n_obj = batch["num_objects"]
    hw_dev = torch.from_numpy(hw).cuda()
    crowd = torch.from_numpy((batch["iscrowd"] != 0).astype(np.uint8)).cuda()
    score, label = K.det_postprocess(cat_pred)
    score_host, label_host = score.cpu().numpy(), label.cpu().numpy()
    stuff = tuple(range(2, 12))
    is_stuff_host = np.zeros(C, np.uint8)
    is_stuff_host[list(stuff)] = 1
    is_stuff = torch.from_numpy(is_stuff_host).cuda()
    selections = {"about 10 kept": float(np.quantile(score_host, 0.9)), "all 100 kept": 0.0}

    # the kernels against the plain-loop reference on the first image, for both selections
    import _mask_raster_ref as RR
    import _panoptic_ref as P
    gt_masks = np.stack([RR.segmentation_mask(records[0]["segmentation"][m], h, w) if m < int(n_obj[0]) else np.zeros((h, w), bool) for m in range(M)])
    equal, kept_counts = True, {}
    for name, thr in selections.items():
        want = P.image_reference(logits_host[0], score_host[0], label_host[0], is_stuff_host, thr, gt_masks, cat_ids_host[0],
                                 (batch["iscrowd"][0] != 0), int(n_obj[0]), C, min_area, h, w)
        gt_bits, _ = K.mask_source_bits(pack["items"], pack["item_off"], pack["kind"], pack["hw"], Hm, Wm)
        gt_pop = K.panoptic_gt_exclusive(gt_bits, cat_ids, num_objects, C)
        seg_of = K.panoptic_select(score, label, thr, C, is_stuff)
        ids, bits, pop = K.panoptic_merge(logits, seg_of, hw_dev, Hm, Wm)
        inter = K.mask_inter(bits, gt_bits, num_objects)
        got = K.panoptic_match(inter, pop, label, seg_of, gt_pop, cat_ids, crowd, num_objects, C, min_area)
        torch.cuda.synchronize()
        equal = equal and np.array_equal(seg_of[0].cpu().numpy(), want["seg_of"]) and np.array_equal(ids[0].cpu().numpy(), P.ids_canvas(want["ids"], Hm, Wm))
        equal = equal and np.array_equal(pop[0].cpu().numpy(), want["pred_pop"]) and np.array_equal(gt_pop[0].cpu().numpy(), want["gt_pop"])
        equal = equal and np.array_equal(inter[0].cpu().numpy(), want["inter"])
        equal = equal and all(np.array_equal(t[0].cpu().numpy(), want[k]) for t, k in zip(got, ("gt_state", "pred_state", "match_inter", "match_union")))
        kept_counts[name] = float((seg_of >= 0).sum().item()) / B

    res = {}
    gt_bits_fresh, _ = K.mask_source_bits(pack["items"], pack["item_off"], pack["kind"], pack["hw"], Hm, Wm)
    dev = {k: torch.from_numpy(v).cuda() for k, v in pack.items()}
    from boosted_detr_amd import _lib
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    pop_out = torch.empty(B, M, dtype=torch.int32, device="cuda")
    det_bits = torch.empty(B, N, Hm, Wm, dtype=torch.int64, device="cuda")

    def k19():
        K.mask_upsample_bits(logits, hw_dev, Hm, Wm, out=det_bits)

    def k20():
        _lib.check(lib.bdetr_mask_source_bits(dev["items"].data_ptr(), dev["items"].numel(), dev["item_off"].data_ptr(), dev["kind"].data_ptr(),
                                              dev["hw"].data_ptr(), B, M, Hm, Wm, gt_bits_fresh.data_ptr(), pop_out.data_ptr(), stream))

    def k25():                                       # in place: after the first call the rows are exclusive already (the same traffic)
        K.panoptic_gt_exclusive(gt_bits_fresh, cat_ids, num_objects, C)

    image_ev = evaluation.CocoImageMaskEvaluator(C)

    def image_update():
        image_ev._kept.clear()
        image_ev.update(cat_pred, logits, cat_ids, pack, num_objects, hw, batch["iscrowd"], batch["area"])

    for fn in (k19, k20, k25, image_update):
        for _ in range(3):
            fn()
    res["K19"] = windows(k19, args.reps, args.inner, True)
    res["K20"] = windows(k20, args.reps, args.inner, True)
    res["K25"] = windows(k25, args.reps, args.inner, True)
    per_selection = {}
    for name, thr in selections.items():
        seg_of = K.panoptic_select(score, label, thr, C, is_stuff)
        _, bits, pop = K.panoptic_merge(logits, seg_of, hw_dev, Hm, Wm)
        gt_pop = K.panoptic_gt_exclusive(gt_bits_fresh, cat_ids, num_objects, C)
        inter = K.mask_inter(bits, gt_bits_fresh, num_objects)
        ev = evaluation.PanopticEvaluator(C, score_threshold=thr, min_area=min_area, stuff_classes=stuff)

        def k23():
            K.panoptic_select(score, label, thr, C, is_stuff)

        def k24():
            K.panoptic_merge(logits, seg_of, hw_dev, Hm, Wm)

        def k24_no_bits():
            K.panoptic_merge(logits, seg_of, hw_dev, Hm, Wm, with_bits=False)

        def k21():
            K.mask_inter(bits, gt_bits_fresh, num_objects)

        def k26():
            K.panoptic_match(inter, pop, label, seg_of, gt_pop, cat_ids, crowd, num_objects, C, min_area)

        def update():
            ev._kept.clear()
            ev.update(cat_pred, logits, cat_ids, pack, num_objects, hw, batch["iscrowd"])

        for fn in (k23, k24, k24_no_bits, k21, k26, update):
            for _ in range(3):
                fn()
        r = {k: windows(fn, args.reps, args.inner, True) for k, fn in (("K23", k23), ("K24", k24), ("K24_no_bits", k24_no_bits), ("K21", k21), ("K26", k26))}
        r["update"] = windows(update, args.reps, args.inner, False)
        r["kept_per_image"] = kept_counts[name]
        r["threshold"] = thr
        per_selection[name] = r
    res["image_update"] = windows(image_update, args.reps, args.inner, False)
    res["image_update_again"] = windows(image_update, args.reps, args.inner, False)

    k24_bytes = B * Hm * Wm * (8 * N + 128)
    for r in per_selection.values():
        r["K24_TB_per_s"] = round(k24_bytes / (r["K24"]["median_ms"] * 1e-3) / 1e12, 3)
    out = {"load": {"batch": B, "queries": N, "gt_rows": M, "objects_per_image": float(np.mean(n_obj)), "image": [h, w], "Hm": Hm, "Wm": Wm, "grid": G,
                    "min_area": min_area, "stuff_classes": len(stuff)},
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner, "gpu_equal_to_reference": bool(equal), "gpu": res,
           "selections": per_selection, "k24_mandatory_bytes": k24_bytes}
    lines = [
        "panoptic quality at image resolution (K23-K26, csrc/panopticmerge.hip) - written by tools/panoptic_eval_bench.py",
        f"device: {out['device']}",
        f"load: batch {B}, {N} queries, {M} ground-truth rows with {out['load']['objects_per_image']:.1f} objects per image (6 polygons of 40 vertices, one crowd",
        f"  RLE), {h} x {w} images: Hm = {Hm}, Wm = {Wm}; logits 3 N(0,1) on the {G} x {G} grid; min_area {min_area}, {len(stuff)} stuff classes",
        f"method: after warm-up, {args.reps} windows of {args.inner} calls each, every window closed by a device synchronise; median (min - max) per call.",
        "  kernels: device-resident operands between two device events.  updates: host clock, nothing read back.",
        f"K23-K26 (with K20, K21) equal to the plain-loop reference on the first image, both selections: {out['gpu_equal_to_reference']}",
        "",
        "the yardstick, same batch:",
        f"  K19 bdetr_mask_upsample_bits (all {N} queries)          {fmt(res['K19'])}",
        f"  CocoImageMaskEvaluator.update                          {fmt(res['image_update'])}",
        f"  CocoImageMaskEvaluator.update, measured again          {fmt(res['image_update_again'])}",
        "shared by both selections:",
        f"  K20 bdetr_mask_source_bits                             {fmt(res['K20'])}",
        f"  K25 bdetr_panoptic_gt_exclusive                        {fmt(res['K25'])}",
    ]
    for name, r in per_selection.items():
        lines += [
            f"selection \"{name}\": score threshold {r['threshold']:.6f}, {r['kept_per_image']:.1f} kept queries per image",
            f"  K23 bdetr_panoptic_select                              {fmt(r['K23'])}",
            f"  K24 bdetr_panoptic_merge                               {fmt(r['K24'])}",
            f"      mandatory bytes (bits and ids written) {k24_bytes} -> {r['K24_TB_per_s']:.3f} TB/s achieved against them",
            f"  K24 without bits (panoptic_segmentation)               {fmt(r['K24_no_bits'])}",
            f"  K21 bdetr_mask_inter on the disjoint sets              {fmt(r['K21'])}",
            f"  K26 bdetr_panoptic_match                               {fmt(r['K26'])}",
            f"  PanopticEvaluator.update                               {fmt(r['update'])}",
        ]
    lines += ["", "json: " + json.dumps(out)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    dest = args.out or os.path.join(ROOT, "profiles", f"panoptic_eval_{time.strftime('%Y-%m-%d')}.txt")
    with open(dest, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
