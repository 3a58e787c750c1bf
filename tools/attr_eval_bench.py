"""Time of one batch of attribute-aware AP (K29-K31, csrc/attrmetric.hip; evaluation.AttributeEvaluator) at a Fashionpedia-like load,
next to the COCO protocol without the gate (evaluation.CocoEvaluator, K16) on the same batch:

  batch 16, 100 queries, 100 ground-truth rows with 7 objects per image, 296 attributes (5 words), 46 + 2 categories, T = F = 10.

What is timed (after warm-up; every window ends in a device synchronise; `reps` windows of `inner` calls, median and spread):
  K29           bdetr_attr_pack on the predictions [B N, A] and on the targets [B M, A], between two device events
  K30 / K16     bdetr_det_match_attr beside bdetr_det_match_coco on the same operands, in the same run, between two device events.
                K30 launches F times the workgroups: the ratio is the number to read
  updates       AttributeEvaluator.update and CocoEvaluator.update on the host clock; neither reads anything back
The kernels' results are compared with the plain-loop reference (tests/_attr_ref.py) on the first two images before anything is timed.
--coco-only times CocoEvaluator.update alone: run it in alternating processes against two builds of the library (BDETR_LIB names
the other one; a library without the K29-K31 symbols is accepted in this mode) to see that the existing path did not move.

The report is printed and written to profiles/attr_eval_<date>.txt (or --out FILE): the committed profile IS this tool's output.

    python tools/attr_eval_bench.py [--reps 20] [--inner 20] [--out FILE] [--coco-only]
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

NEW_SYMBOLS = ("bdetr_attr_pack", "bdetr_det_match_attr", "bdetr_mask_match_attr")


def fmt(r):
    return f"{r['median_ms']:10.4f} ms  ({r['min_ms']:.4f} - {r['max_ms']:.4f})"


def make_load(B, N, M, C, A, objects, seed=2024):
    """Ground truths at random, 0 to 4 of 8 live attributes each; a detection is a jittered ground truth of its image with that
    ground truth's attributes, one more or less, or a fresh draw (tests/_attr_ref.py's recipe)."""
    import _attr_ref as AR
    c = AR.make_box_case(seed, B, N, objects, A, C, [objects] * B, AR.THR10, AR.THR10, (480, 640), AR.R.COCO_AREA_RANGES, crowd_fraction=0.1)
    for key, fill in (("gt_box", -10.0), ("gt_label", 0), ("gt_attr", 0.0), ("gt_crowd", 0)):      # the rows past num_objects are padding
        pad = np.full((B, M - objects) + c[key].shape[2:], fill, c[key].dtype)
        c[key] = np.ascontiguousarray(np.concatenate([c[key], pad], 1))
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--coco-only", action="store_true", help="time CocoEvaluator.update alone (to compare two builds of the library)")
    ap.add_argument("--out", default=None, help="where the report goes (default: profiles/attr_eval_<date>.txt)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU path: no GPU, no number"
    from mask_targets_bench import windows
    from boosted_detr_amd import _lib
    if args.coco_only and os.environ.get("BDETR_LIB"):
        for name in NEW_SYMBOLS:                   # the other build may be one from before K29-K31
            _lib.SIGNATURES.pop(name, None)
    from boosted_detr_amd import evaluation
    from boosted_detr_amd import kernels as K
    B, N, M, C, A, objects = args.batch, 100, 100, 48, 296, 7
    c = make_load(B, N, M, C, A, objects)
    rng = np.random.default_rng(7)
    cat_host = rng.random((B, N, C)).astype(np.float32) * 0.5
    np.put_along_axis(cat_host, c["label"][..., None].astype(np.int64), (0.5 + 0.5 * rng.random((B, N, 1))).astype(np.float32), 2)
    cat_host[..., :2] = 0.0
    cat_pred = torch.from_numpy(cat_host).cuda()
    attribute_pred, attribute_hot = torch.from_numpy(c["det_attr"]).cuda(), torch.from_numpy(c["gt_attr"]).cuda()
    box_pred, bbox = torch.from_numpy(c["box"]).cuda(), torch.from_numpy(c["gt_box"]).cuda()
    cat_ids, num_objects = torch.from_numpy(c["gt_label"]).cuda(), torch.from_numpy(c["num_objects"]).cuda()
    iscrowd, hw = c["gt_crowd"].astype(np.int32), (480, 640)
    coco_ev = evaluation.CocoEvaluator(C)

    def coco_update():
        coco_ev._kept.clear()
        coco_ev.update(cat_pred, box_pred, cat_ids, bbox, num_objects, iscrowd, None, hw)

    for _ in range(5):
        coco_update()
    if args.coco_only:
        r = windows(coco_update, args.reps, args.inner, False)
        print(f"CocoEvaluator.update  {fmt(r)}  library: {_lib.lib_path()}")
        print("json: " + json.dumps({"coco_update": r, "library": str(_lib.lib_path()), "device": torch.cuda.get_device_name(0), "reps": args.reps,
                                     "inner": args.inner}))
        return

    import _attr_ref as AR
    thr = f1s = AR.THR10
    score, label = K.det_postprocess(cat_pred)
    det_attr, det_count = K.attr_pack(attribute_pred)
    gt_attr, gt_attr_count = K.attr_pack(attribute_hot)
    crowd = torch.from_numpy(c["gt_crowd"]).cuda()
    hw_dev = torch.from_numpy(c["image_hw"]).cuda()
    ranges = torch.from_numpy(np.asarray(list(evaluation.COCO_AREA_RANGES.values()), np.float64)).cuda()
    gt_count = torch.zeros(4, C, dtype=torch.int32, device="cuda")

    def k30():
        return K.det_match_attr(score, label, box_pred, det_attr, det_count, cat_ids, bbox, gt_attr, gt_attr_count, crowd, None, num_objects, hw_dev,
                                ranges, thr, f1s, 1.0, C, 100, gt_count)

    def k16():
        return K.det_match_coco(score, label, box_pred, cat_ids, bbox, crowd, None, num_objects, hw_dev, ranges, thr, C, 100, gt_count)

    got = [t.cpu().numpy() for t in k30()]
    torch.cuda.synchronize()
    score_h, label_h = score.cpu().numpy(), label.cpu().numpy()
    equal, redirected = True, 0
    for b in range(2):
        per_f, k = AR.match_image(score_h[b], label_h[b], c["box"][b], c["det_attr"][b], c["gt_label"][b], c["gt_box"][b], c["gt_attr"][b], c["gt_crowd"][b],
                                  None, c["num_objects"][b], 480, 640, thr, f1s, 1.0, AR.R.COCO_AREA_RANGES, 100, C)
        redirected += k["redirected"]
        equal = equal and bool(np.array_equal(got[0][b], per_f[0]["order"])) and all(
            np.array_equal(got[4][f, a, b], per_f[f]["matched_gt"][a]) and
            np.array_equal(got[2][f, a, b].view(np.uint16), AR.R.pack_bits(per_f[f]["keep"], per_f[f]["tp"][a])) for f in range(len(f1s)) for a in range(4))

    def k29_pred():
        K.attr_pack(attribute_pred)

    def k29_gt():
        K.attr_pack(attribute_hot)

    attr_ev = evaluation.AttributeEvaluator(C, A)

    def attr_update():
        attr_ev._kept.clear()
        attr_ev.update(cat_pred, attribute_pred, box_pred, cat_ids, attribute_hot, bbox, num_objects, iscrowd, None, hw)

    for fn in (k29_pred, k29_gt, k30, k16, attr_update, coco_update):
        for _ in range(3):
            fn()
    res = {name: windows(fn, args.reps, args.inner, True) for name, fn in (("K29_pred", k29_pred), ("K29_gt", k29_gt), ("K30", k30), ("K16", k16),
                                                                           ("K30_again", k30), ("K16_again", k16))}
    res["attr_update"] = windows(attr_update, args.reps, args.inner, False)
    res["coco_update"] = windows(coco_update, args.reps, args.inner, False)
    res["attr_update_again"] = windows(attr_update, args.reps, args.inner, False)
    res["coco_update_again"] = windows(coco_update, args.reps, args.inner, False)
    ratio = res["K30"]["median_ms"] / res["K16"]["median_ms"]
    pack_bytes = 4 * B * N * A + 8 * B * N * ((A + 63) // 64) + 4 * B * N
    out = {"load": {"batch": B, "queries": N, "gt_rows": M, "objects_per_image": objects, "classes": C, "attributes": A, "T": len(thr), "F": len(f1s),
                    "lds_bytes": K.attr_match_lds_bytes(N, M, (A + 63) // 64), "workgroups_K30": B * 4 * len(f1s), "workgroups_K16": B * 4},
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner, "gpu_equal_to_reference": bool(equal),
           "redirected_in_two_images": int(redirected), "gpu": res, "k30_over_k16": round(ratio, 3),
           "k29_pred_GB_per_s": round(pack_bytes / (res["K29_pred"]["median_ms"] * 1e-3) / 1e9, 1)}
    lines = [
        "attribute-aware AP (K29-K31, csrc/attrmetric.hip) - written by tools/attr_eval_bench.py",
        f"device: {out['device']}",
        f"load: batch {B}, {N} queries, {M} ground-truth rows with {objects} objects per image, {C} classes, {A} attributes ({(A + 63) // 64} words), T = {len(thr)},",
        f"  F = {len(f1s)}; K30 stages {out['load']['lds_bytes']} bytes of LDS per workgroup and launches {out['load']['workgroups_K30']} workgroups, K16 {out['load']['workgroups_K16']}",
        f"method: after warm-up, {args.reps} windows of {args.inner} calls each, every window closed by a device synchronise; median (min - max) per call.",
        "  kernels: device-resident operands between two device events (output allocation included).  updates: host clock, nothing read back.",
        f"K30 equal to the plain-loop reference on the first two images: {out['gpu_equal_to_reference']} ({redirected} detections redirected by the gate there)",
        "",
        f"  K29 bdetr_attr_pack, predictions [{B * N}, {A}]          {fmt(res['K29_pred'])}   {out['k29_pred_GB_per_s']} GB/s",
        f"  K29 bdetr_attr_pack, targets [{B * M}, {A}]              {fmt(res['K29_gt'])}",
        f"  K30 bdetr_det_match_attr (T x F = {len(thr)} x {len(f1s)})             {fmt(res['K30'])}",
        f"  K16 bdetr_det_match_coco, same operands             {fmt(res['K16'])}",
        f"  K30, measured again                                 {fmt(res['K30_again'])}",
        f"  K16, measured again                                 {fmt(res['K16_again'])}",
        f"      K30 / K16 = {ratio:.2f} with {len(f1s)} times the workgroups",
        f"  AttributeEvaluator.update                           {fmt(res['attr_update'])}",
        f"  CocoEvaluator.update, same batch                    {fmt(res['coco_update'])}",
        f"  AttributeEvaluator.update, measured again           {fmt(res['attr_update_again'])}",
        f"  CocoEvaluator.update, measured again                {fmt(res['coco_update_again'])}",
        "",
        "json: " + json.dumps(out),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    dest = args.out or os.path.join(ROOT, "profiles", f"attr_eval_{time.strftime('%Y-%m-%d')}.txt")
    with open(dest, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
