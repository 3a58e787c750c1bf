"""Time of one batch of mask AP at image resolution (K19-K22, csrc/maskimage.hip; evaluation.CocoImageMaskEvaluator) at a COCO-like
load, next to the grid path (evaluation.CocoMaskEvaluator, K15 / K17) on the same batch:

  batch 16, 100 queries, 100 ground-truth rows, 480 x 640 images; per image 6 polygon objects of about 40 vertices and one crowd RLE
  of about 3,000 runs (tools/mask_targets_bench.py's generator), logits 3 N(0,1) on the 23 x 23 grid.

What is timed (after warm-up; every window ends in a device synchronise; `reps` windows of `inner` calls, median and spread):
  K19 .. K22    each kernel alone on device-resident operands, between two device events
  image update  CocoImageMaskEvaluator.update: host checks, two host-to-device copies, det_postprocess and the four kernels; host clock
  grid update   CocoMaskEvaluator.update on the same batch (its 23 x 23 targets from pipeline.mask_targets); host clock
For K21 the achieved bytes per second are set against its mandatory bytes, sum over the images of 8 Hm Wm (N + num_objects).
Neither update reads anything back: the only synchronisation is the one that closes a window.
The kernels' results are compared with the NumPy references (tests/_mask_image_ref.py, tests/_mask_raster_ref.py) on the first two
images before anything is timed.  --grid-only times the grid update alone (to compare two builds of the library).

The report is printed and written to profiles/mask_image_eval_<date>.txt (or --out FILE): the committed profile IS this tool's output.

    python tools/mask_image_eval_bench.py [--reps 20] [--inner 20] [--out FILE] [--grid-only]
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
    ap.add_argument("--grid-only", action="store_true", help="time CocoMaskEvaluator.update alone")
    ap.add_argument("--out", default=None, help="where the report goes (default: profiles/mask_image_eval_<date>.txt)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU path: no GPU, no number"
    from mask_targets_bench import make_records, windows
    from boosted_detr_amd import evaluation, pipeline
    from boosted_detr_amd import kernels as K
    B, N, M, C, G, h, w = args.batch, 100, 100, 92, 23, 480, 640
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
    cat_ids = torch.from_numpy(rng.integers(2, C, (B, M)).astype(np.int32)).cuda()
    num_objects = torch.from_numpy(batch["num_objects"].astype(np.int32)).cuda()
    grid_masks = pipeline.mask_targets(pack, G)["masks"]
    grid_ev = evaluation.CocoMaskEvaluator(C)

    def grid_update():
        grid_ev._kept.clear()
        grid_ev.update(cat_pred, logits, cat_ids, grid_masks, num_objects, batch["iscrowd"], batch["area"], hw)

    for _ in range(5):
        grid_update()
    if args.grid_only:
        r = windows(grid_update, args.reps, args.inner, False)
        print(f"grid update (CocoMaskEvaluator.update)  {fmt(r)}")
        print("json: " + json.dumps({"grid_update": r, "device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner}))
        return

    import _mask_image_ref as MI
    import _mask_raster_ref as RR
    hw_dev = torch.from_numpy(hw).cuda()
    pix = torch.from_numpy((hw[:, 0] * hw[:, 1]).astype(np.int32)).cuda()
    det_bits, det_pop = K.mask_upsample_bits(logits, hw_dev, Hm, Wm)
    gt_bits, gt_pop = K.mask_source_bits(pack["items"], pack["item_off"], pack["kind"], pack["hw"], Hm, Wm)
    inter = K.mask_inter(det_bits, gt_bits, num_objects)
    torch.cuda.synchronize()
    db, gb = det_bits[:2].cpu().numpy().view(np.uint64), gt_bits[:2].cpu().numpy().view(np.uint64)
    n_obj = batch["num_objects"]
    equal = all(np.array_equal(db[b, n], MI.pack(MI.upsample_mask(logits_host[b, n], h, w), Hm, Wm)) for b in range(2) for n in range(0, N, 9))
    equal = equal and all(np.array_equal(gb[b, m], MI.pack(RR.segmentation_mask(records[b]["segmentation"][m], h, w), Hm, Wm))
                          for b in range(2) for m in range(int(n_obj[b])))
    equal = equal and bool(np.array_equal(inter[:2].cpu().numpy(), MI.inter(db, gb, n_obj[:2])))

    dev = {k: torch.from_numpy(v).cuda() for k, v in pack.items()}
    from boosted_detr_amd import _lib
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    score, label = K.det_postprocess(cat_pred)
    crowd = torch.from_numpy((batch["iscrowd"] != 0).astype(np.uint8)).cuda()
    ranges = torch.from_numpy(np.asarray(list(evaluation.COCO_AREA_RANGES.values()), np.float64)).cuda()
    gt_count = torch.zeros(4, C, dtype=torch.int32, device="cuda")
    thr = np.linspace(0.5, 0.95, 10)
    pop_out = torch.empty(B, M, dtype=torch.int32, device="cuda")

    def k19():
        K.mask_upsample_bits(logits, hw_dev, Hm, Wm, out=det_bits)

    def k20():
        _lib.check(lib.bdetr_mask_source_bits(dev["items"].data_ptr(), dev["items"].numel(), dev["item_off"].data_ptr(), dev["kind"].data_ptr(),
                                              dev["hw"].data_ptr(), B, M, Hm, Wm, gt_bits.data_ptr(), pop_out.data_ptr(), stream))

    def k21():
        K.mask_inter(det_bits, gt_bits, num_objects)

    def k22():
        K.mask_match_coco_inter(score, label, inter, det_pop, cat_ids, gt_pop, crowd, None, num_objects, hw_dev, pix, ranges, thr, C, 100, gt_count)

    image_ev = evaluation.CocoImageMaskEvaluator(C)

    def image_update():
        image_ev._kept.clear()
        image_ev.update(cat_pred, logits, cat_ids, pack, num_objects, hw, batch["iscrowd"], batch["area"])

    for fn in (k19, k20, k21, k22, image_update, grid_update):
        for _ in range(3):
            fn()
    res = {name: windows(fn, args.reps, args.inner, True) for name, fn in (("K19", k19), ("K20", k20), ("K21", k21), ("K22", k22))}
    res["image_update"] = windows(image_update, args.reps, args.inner, False)
    res["grid_update"] = windows(grid_update, args.reps, args.inner, False)
    res["grid_update_again"] = windows(grid_update, args.reps, args.inner, False)
    t0 = time.perf_counter()
    for _ in range(20):
        image_ev.check_batch(pack, hw, N)
        K.check_source_pack(pack["items"], pack["item_off"], pack["kind"], pack["hw"], Hm, Wm)
    check_ms = (time.perf_counter() - t0) * 1e3 / 20
    floor_bytes = int(sum(8 * Hm * Wm * (N + int(n)) for n in n_obj))
    k21_tbps = floor_bytes / (res["K21"]["median_ms"] * 1e-3) / 1e12
    out = {"load": {"batch": B, "queries": N, "gt_rows": M, "objects_per_image": float(np.mean(n_obj)), "image": [h, w], "Hm": Hm, "Wm": Wm, "grid": G,
                    "bitmask_bytes": 8 * Hm * Wm * B * (N + M), "set_det_pixels": int(det_pop.sum()), "set_gt_pixels": int(gt_pop.sum())},
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner, "gpu_equal_to_reference": bool(equal), "gpu": res,
           "k21": {"mandatory_bytes": floor_bytes, "achieved_TB_per_s": round(k21_tbps, 3)}, "host": {"checks_ms": round(check_ms, 3)}}
    lines = [
        "mask AP at image resolution (K19-K22, csrc/maskimage.hip) - written by tools/mask_image_eval_bench.py",
        f"device: {out['device']}",
        f"load: batch {B}, {N} queries, {M} ground-truth rows with {out['load']['objects_per_image']:.1f} objects per image (6 polygons of 40 vertices, one crowd",
        f"  RLE), {h} x {w} images: Hm = {Hm}, Wm = {Wm}, {out['load']['bitmask_bytes'] / 2 ** 20:.1f} MiB of bitmasks per batch; logits 3 N(0,1) on the {G} x {G} grid",
        f"method: after warm-up, {args.reps} windows of {args.inner} calls each, every window closed by a device synchronise; median (min - max) per call.",
        "  K19-K22: each kernel on device-resident operands between two device events.  updates: host clock, nothing read back.",
        f"K19, K20, K21 equal to the NumPy references on the first two images: {out['gpu_equal_to_reference']}",
        "",
        f"  K19 bdetr_mask_upsample_bits                        {fmt(res['K19'])}",
        f"  K20 bdetr_mask_source_bits                          {fmt(res['K20'])}",
        f"  K21 bdetr_mask_inter (with the zeroing of inter)    {fmt(res['K21'])}",
        f"      mandatory bytes {floor_bytes} -> {k21_tbps:.3f} TB/s achieved against them",
        f"  K22 bdetr_mask_match_coco_inter                     {fmt(res['K22'])}",
        f"  CocoImageMaskEvaluator.update (image resolution)    {fmt(res['image_update'])}",
        f"    of which the host checks of the pack              {check_ms:10.4f} ms",
        f"  CocoMaskEvaluator.update (grid), same batch         {fmt(res['grid_update'])}",
        f"  CocoMaskEvaluator.update (grid), measured again     {fmt(res['grid_update_again'])}",
        "",
        "json: " + json.dumps(out),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    dest = args.out or os.path.join(ROOT, "profiles", f"mask_image_eval_{time.strftime('%Y-%m-%d')}.txt")
    with open(dest, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
