"""Time of one batch of mask targets (K18, csrc/maskraster.hip) at a COCO-like load, next to the host NumPy reference of the same
rule (tests/_mask_raster_ref.py) on the same data:

  batch 16, 480 x 640 sources, per image 7 polygon objects of about 40 vertices and one crowd RLE of about 3,000 runs (given as the
  compressed string), placed on a 640 x 640 canvas by Augmentations.draw.

What is timed (after warm-up; every window ends in a device synchronise; `reps` windows of `inner` calls, median and spread):
  kernel        bdetr_mask_targets alone on device-resident operands, between two device events
  mask_targets  pipeline.mask_targets(pack, placement): the host check of the pack, ONE host-to-device copy, the launch; host clock
  pack          pipeline.pad_annotations(records, with_masks=True): decoding the RLE strings, snapping, packing; host clock, no GPU
  reference     the plain-loop NumPy reference for the whole batch, once; host clock, no GPU
The GPU result is compared bit for bit with the reference before anything is timed.

The report is printed and written to profiles/mask_targets_<date>.txt (or --out FILE): the committed profile IS this tool's output.

    python tools/mask_targets_bench.py [--reps 20] [--inner 50] [--out FILE]
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


def make_records(B, h, w, polygons, vertices, runs, seed):
    from boosted_detr_amd import pipeline
    rng = np.random.default_rng(seed)
    records = []
    for _ in range(B):
        segs = []
        for _ in range(polygons):
            cx, cy, r = rng.uniform(0.1 * w, 0.9 * w), rng.uniform(0.1 * h, 0.9 * h), rng.uniform(15, 140)
            ang = np.sort(rng.uniform(0, 2 * np.pi, vertices))
            rad = r * rng.uniform(0.6, 1.0, vertices)
            segs.append([np.round(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=-1), 2).reshape(-1).tolist()])
        x0 = int(rng.integers(0, w // 2))                                     # the crowd region: a band of columns, short vertical runs
        lo, hi = x0 * h, (x0 + w // 2) * h
        cuts = np.unique(rng.integers(lo, hi, 2 * runs))
        counts = np.diff(np.concatenate([[0], cuts, [h * w]])).tolist()
        segs.append({"size": [h, w], "counts": pipeline.encode_rle_counts(counts)})
        n = len(segs)
        records.append({"height": h, "width": w, "bbox": [[0.1, 0.1, 0.5, 0.5]] * n, "category": [["x"]] * n, "segmentation": segs})
    return records


def windows(fn, reps, inner, device_events):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        if device_events:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b) / inner)
        else:
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3 / inner)
    return {"median_ms": round(float(np.median(out)), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None, help="where the report goes (default: profiles/mask_targets_<date>.txt)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU path: no GPU, no number"
    import _mask_raster_ref as R
    from boosted_detr_amd import _lib, pipeline
    from boosted_detr_amd import kernels as K
    B, h, w, H, W, G = args.batch, 480, 640, 640, 640, 23
    records = make_records(B, h, w, polygons=7, vertices=40, runs=3000, seed=2024)
    t0 = time.perf_counter()
    for _ in range(5):
        batch = pipeline.pad_annotations(records, with_masks=True)
    pack_ms = (time.perf_counter() - t0) * 1e3 / 5
    pack = batch["segments"]
    p = pipeline.Augmentations(seed=7).draw(B, H, W)
    place = np.stack([np.full(B, H), np.full(B, W), p["new_h"], p["new_w"], p["off_h"], p["off_w"]], axis=-1).astype(np.int32)

    t0 = time.perf_counter()
    want = np.zeros((B, 8, G, G), np.float32)
    want_area = np.zeros((B, 8), np.int32)
    for b in range(B):
        for m, seg in enumerate(records[b]["segmentation"]):
            want[b, m], want_area[b, m] = R.target(R.segmentation_mask(seg, h, w), G, tuple(int(v) for v in place[b]))
    ref_ms = (time.perf_counter() - t0) * 1e3

    got = pipeline.mask_targets(pack, G, place)
    torch.cuda.synchronize()
    equal = bool(np.array_equal(got["masks"].cpu().numpy().view(np.uint32), want.view(np.uint32))
                 and np.array_equal(got["mask_area"].cpu().numpy(), want_area))

    dev = {k: torch.from_numpy(v).cuda() for k, v in dict(pack, placement=place).items()}
    masks = torch.empty(B, 8, G, G, device="cuda")
    area = torch.empty(B, 8, dtype=torch.int32, device="cuda")
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream

    def kernel():
        _lib.check(lib.bdetr_mask_targets(dev["items"].data_ptr(), dev["items"].numel(), dev["item_off"].data_ptr(), dev["kind"].data_ptr(),
                                          dev["hw"].data_ptr(), dev["placement"].data_ptr(), B, 8, G, masks.data_ptr(), area.data_ptr(), stream))

    def full():
        pipeline.mask_targets(pack, G, place)

    for _ in range(5):
        kernel()
        full()
    res = {"kernel": windows(kernel, args.reps, args.inner, True), "mask_targets": windows(full, args.reps, args.inner, False)}
    t0 = time.perf_counter()
    for _ in range(20):
        K.check_mask_pack(pack["items"], pack["item_off"], pack["kind"], pack["hw"], place, G)
    check_ms = (time.perf_counter() - t0) * 1e3 / 20
    out = {"load": {"batch": B, "source": [h, w], "canvas": [H, W], "grid": G, "objects_per_image": 8, "polygon_vertices": 40,
                    "rle_one_runs_per_image": int(np.mean([(pack["item_off"][b * 8 + 8] - pack["item_off"][b * 8 + 7]) // 2 for b in range(B)])),
                    "items_int32": int(pack["items"].size), "set_pixels": int(want_area.sum())},
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner,
           "gpu_bit_equal_to_reference": equal, "gpu": res,
           "host": {"pack_ms": round(pack_ms, 3), "check_mask_pack_ms": round(check_ms, 3), "numpy_reference_ms": round(ref_ms, 1)}}
    g, hst = out["gpu"], out["host"]
    head_ms = 2.1                                        # what the mask head adds to the configs[4] step (profiles/README.md)
    lines = [
        "mask targets (K18, csrc/maskraster.hip) - written by tools/mask_targets_bench.py",
        f"device: {out['device']}",
        f"load: batch {B}, {h} x {w} sources on a {H} x {W} canvas, grid {G}; per image 7 polygon objects of 40 vertices and one crowd RLE of",
        f"  {out['load']['rle_one_runs_per_image']} one-runs on average, given as the compressed string; {out['load']['items_int32']} int32 items in the pack, "
        f"{out['load']['set_pixels']} set source pixels; placement from Augmentations(seed=7).draw",
        f"method: after warm-up, {args.reps} windows of {args.inner} calls each, every window closed by a device synchronise; median (min - max) per call.",
        "  kernel: bdetr_mask_targets on device-resident operands between two device events.  mask_targets: pipeline.mask_targets(pack,",
        "  placement) = host check of the pack + one host-to-device copy + the launch, host clock.  host rows: host clock, no GPU.",
        f"GPU result bit-equal to the NumPy reference on this data: {out['gpu_bit_equal_to_reference']}",
        "",
        f"  kernel (device events)                              {g['kernel']['median_ms']:10.4f} ms  ({g['kernel']['min_ms']:.4f} - {g['kernel']['max_ms']:.4f})",
        f"  pipeline.mask_targets (check + copy + launch)       {g['mask_targets']['median_ms']:10.4f} ms  ({g['mask_targets']['min_ms']:.4f} - {g['mask_targets']['max_ms']:.4f})",
        f"    of which kernels.check_mask_pack on the host      {hst['check_mask_pack_ms']:10.4f} ms",
        f"  host NumPy reference (tests/_mask_raster_ref.py)    {hst['numpy_reference_ms']:10.1f} ms  (whole batch, once)",
        f"  pad_annotations(with_masks=True), host packing      {hst['pack_ms']:10.3f} ms  (decodes the compressed RLE strings in Python)",
        "",
        f"against the {head_ms} ms the mask head adds at configs[4]: the kernel is {g['kernel']['median_ms'] / head_ms:.2f}x of it, "
        f"pipeline.mask_targets {g['mask_targets']['median_ms'] / head_ms:.2f}x",
        "",
        "json: " + json.dumps(out),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    dest = args.out or os.path.join(ROOT, "profiles", f"mask_targets_{time.strftime('%Y-%m-%d')}.txt")
    with open(dest, "w") as f:
        f.write(text)

if __name__ == "__main__":
    main()
