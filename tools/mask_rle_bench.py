"""Time of the run-length encoder for predicted masks (K27 / K28, csrc/maskrle.hip; kernels.mask_rle_encode) at the load of the other
evaluation rows of the README:

  batch 16, 100 queries, 480 x 640 images; the masks are K19's (bdetr_mask_upsample_bits) on logits 3 N(0,1) on the 23 x 23 grid.
  A second case replaces every mask by a checkerboard: the largest output K28 can be asked for.

What is timed (after warm-up; every window ends in a device synchronise; `reps` windows of `inner` calls, median and spread):
  K19, K27, K28     each kernel alone on device-resident operands and preallocated outputs, between two device events, in one run
  mask_rle_encode   kernels.mask_rle_encode: K27, the prefix sum, the read-back of the total, K28; host clock
  runs to host      (counts, offset).cpu(): what crosses the bus
  host alternative  bits.cpu() of the whole batch, plus a vectorised NumPy encoder on ONE image's masks times the batch size; host clock
Bytes: K27 must read every word of the image's rows once, 8 h Wm per mask, and writes 4 bytes per mask; K28 must read the same words
and write 4 bytes per run length (it reads the words twice, the second time through the caches: the rate is set against the
mandatory bytes).  Before anything is timed the encoder's output is compared with the NumPy encoder on the first image's masks and
with the plain-loop reference (tests/_rle_ref.py) on three of them.

The report is printed and written to profiles/mask_rle_<date>.txt (or --out FILE): the committed profile IS this tool's output.

    python tools/mask_rle_bench.py [--reps 20] [--inner 20] [--out FILE]

A window of K27 is 10 x inner calls: the kernel is some 10 microseconds long, near what a launch from Python costs, so the event
timing is an upper bound of its time.  The kernels' own times come from a profiler run of the same calls and nothing else:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mask_rle_bench.py --trace-loop 50
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


def numpy_encode(words, h, w):
    """One mask uint64 [Hm, Wm] -> run lengths, vectorised: what a user would write on the host copy of the bitmasks."""
    rows = np.unpackbits(np.ascontiguousarray(words[:h]).view(np.uint8), axis=1, bitorder="little")[:, :w]
    flat = rows.flatten(order="F")
    pos = np.flatnonzero(np.diff(flat, prepend=np.uint8(0)))
    return np.diff(np.concatenate([[0], pos, [h * w]])).astype(np.int32) if pos.size else np.asarray([h * w], np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None, help="where the report goes (default: profiles/mask_rle_<date>.txt)")
    ap.add_argument("--trace-loop", type=int, default=0, help="only launch K19, K27 and K28 this many times on the K19 masks (for a profiler run)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU path: no GPU, no number"
    import _rle_ref as RL
    from mask_targets_bench import windows
    from boosted_detr_amd import _lib
    from boosted_detr_amd import kernels as K
    B, N, G, h, w = args.batch, 100, 23, 480, 640
    hw = np.tile(np.asarray([[h, w]], np.int32), (B, 1))
    Hm, Wm = K.mask_layout(hw)
    rng = np.random.default_rng(7)
    logits = torch.from_numpy((3.0 * rng.standard_normal((B, N, G, G))).astype(np.float32)).cuda()
    hw_dev = torch.from_numpy(hw).cuda()
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    upsampled, pop = K.mask_upsample_bits(logits, hw_dev, Hm, Wm)
    row = torch.tensor([0x5555555555555555, -0x5555555555555556], dtype=torch.int64, device="cuda")      # 0x5555..., 0xAAAA... as int64
    checker = row[torch.arange(Hm, device="cuda") % 2][None, None, :, None].expand(B, N, Hm, Wm).contiguous()
    mask_bytes = 8 * h * Wm * B * N
    out = {"load": {"batch": B, "queries": N, "image": [h, w], "Hm": Hm, "Wm": Wm, "grid": G, "bitmask_bytes": 8 * Hm * Wm * B * N},
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner, "cases": {}}
    lines = [
        "run-length encoding of predicted masks (K27 / K28, csrc/maskrle.hip) - written by tools/mask_rle_bench.py",
        f"device: {out['device']}",
        f"load: batch {B}, {N} queries, {h} x {w} images: Hm = {Hm}, Wm = {Wm}, {out['load']['bitmask_bytes'] / 1e6:.1f} MB of bitmasks per batch",
        "method: after warm-up, windows of `inner` calls each, every window closed by a device synchronise; median (min - max) per call.",
        "  K19, K27, K28: each kernel on device-resident operands and preallocated outputs between two device events, in this one run.",
        "  mask_rle_encode, the copies and the host alternative: host clock.",
        "  K21 (bdetr_mask_inter) reads the same bitmasks in 0.026 ms, 2.5 TB/s (profiles/mask_image_eval_*.txt): the class K27 belongs to.",
    ]
    for name, bits, reps, inner in (("K19 masks", upsampled, args.reps, args.inner), ("checkerboard", checker, max(3, args.reps // 4), max(2, args.inner // 10))):
        counts, offset = K.mask_rle_encode(bits, hw_dev, max_bytes=1 << 33)
        torch.cuda.synchronize()
        total = int(counts.numel())
        got, off = counts.cpu().numpy(), offset.cpu().numpy()
        first = bits[0].cpu().numpy().view(np.uint64)
        equal = all(np.array_equal(got[off[n]:off[n + 1]], numpy_encode(first[n], h, w)) for n in range(N))
        equal = equal and all(got[off[n]:off[n + 1]].tolist() == RL.encode_bits(first[n], h, w) for n in (0, N // 2, N - 1))
        n_counts = torch.empty(B, N, dtype=torch.int32, device="cuda")

        def k19():
            K.mask_upsample_bits(logits, hw_dev, Hm, Wm, out=upsampled)

        def k27():
            _lib.check(lib.bdetr_mask_rle_count(bits.data_ptr(), hw_dev.data_ptr(), None, B, N, Hm, Wm, n_counts.data_ptr(), stream))

        def k28():
            _lib.check(lib.bdetr_mask_rle_encode(bits.data_ptr(), hw_dev.data_ptr(), None, offset.data_ptr(), B, N, Hm, Wm, total,
                                                 counts.data_ptr(), stream))

        def whole():
            K.mask_rle_encode(bits, hw_dev, max_bytes=1 << 33)

        def runs_to_host():
            counts.cpu(), offset.cpu()

        for fn in (k19, k27, k28, whole):
            for _ in range(3):
                fn()
        if args.trace_loop:
            for fn in (k19, k27, k28):
                for _ in range(args.trace_loop):
                    fn()
            torch.cuda.synchronize()
            return
        res = {"K19": windows(k19, reps, inner, True) if bits is upsampled else None, "K27": windows(k27, reps, 10 * inner, True),
               "K28": windows(k28, reps, inner, True), "mask_rle_encode": windows(whole, reps, inner, False),
               "runs_to_host": windows(runs_to_host, max(3, reps // 4), 1, False)}
        torch.cuda.synchronize()
        again = torch.empty_like(counts)
        _lib.check(lib.bdetr_mask_rle_encode(bits.data_ptr(), hw_dev.data_ptr(), None, offset.data_ptr(), B, N, Hm, Wm, total, again.data_ptr(), stream))
        equal = equal and bool(torch.equal(again, counts)) and bool(np.array_equal(n_counts.cpu().numpy().reshape(-1), np.diff(off)))
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            copied = bits.cpu().numpy().view(np.uint64)
            t1 = time.perf_counter()
            for n in range(N):
                numpy_encode(copied[0, n], h, w)
            host.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3 * B))
        copy_ms, encode_ms = (float(np.median([v[k] for v in host])) for k in (0, 1))
        k27_bytes, k28_bytes = mask_bytes + 4 * B * N, mask_bytes + 4 * total + 8 * (B * N + 1)
        rate = {"K27_GB_per_s": round(k27_bytes / (res["K27"]["median_ms"] * 1e-3) / 1e9, 1),
                "K28_GB_per_s": round(k28_bytes / (res["K28"]["median_ms"] * 1e-3) / 1e9, 1)}
        out["cases"][name] = {"total_counts": total, "counts_bytes": 4 * total, "set_pixels": int(pop.sum()) if bits is upsampled else B * N * h * w // 2,
                              "equal_to_reference": bool(equal), "gpu": res, "mandatory_bytes": {"K27": k27_bytes, "K28": k28_bytes}, "rate": rate,
                              "host_alternative_ms": {"bits_to_host": round(copy_ms, 2), "numpy_encode_scaled": round(encode_ms, 2)},
                              "windows": [reps, inner]}
        lines += [
            "",
            f"case: {name} - {total} run lengths per batch ({total / (B * N):.1f} per mask, {4 * total / 1e6:.2f} MB against {mask_bytes / 1e6:.1f} MB of bitmask rows); "
            f"{reps} windows of {inner} calls (K27: {10 * inner})",
            f"  output equal to the NumPy encoder (first image) and the plain-loop reference (3 masks), two calls bit-identical: {bool(equal)}",
        ]
        if res["K19"] is not None:
            lines.append(f"  K19 bdetr_mask_upsample_bits (writes these masks)   {fmt(res['K19'])}")
        lines += [
            f"  K27 bdetr_mask_rle_count                            {fmt(res['K27'])}",
            f"      mandatory bytes {k27_bytes} -> {rate['K27_GB_per_s']:.1f} GB/s",
            f"  K28 bdetr_mask_rle_encode                           {fmt(res['K28'])}",
            f"      mandatory bytes {k28_bytes} (read once + written) -> {rate['K28_GB_per_s']:.1f} GB/s",
            f"  kernels.mask_rle_encode (K27, prefix sum, read-back of the total, K28)   {fmt(res['mask_rle_encode'])}",
            f"  (counts, offset) to the host                        {fmt(res['runs_to_host'])}",
            f"  host alternative: bits.cpu() {copy_ms:.2f} ms + NumPy encoder {encode_ms:.2f} ms (one image's {N} masks x {B})",
        ]
    lines += ["", "json: " + json.dumps(out)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    dest = args.out or os.path.join(ROOT, "profiles", f"mask_rle_{time.strftime('%Y-%m-%d')}.txt")
    with open(dest, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
