#!/usr/bin/env python3
"""Time of the fused attention core with and without a mask (csrc/attention.hip, include/bdetr.h K32 / K33).

    python tools/attention_mask_bench.py [--out FILE]
        forward + backward (dvec + dQ + dK/dV) at B = 16, h = 8, 400 x 400 (encoder self-attention) and 100 x 400 (decoder
        cross-attention) under the 'split' policy, each of: unmasked, key-only f32 [B,1,1,k], key-only bool, full f32 [B,h,q,k],
        full bool - all in THIS process, interleaved window by window.  Each masked time is reported beside the unmasked time of
        the same run and beside the time the mask's own bytes take at the HBM rate (forward reads the mask once, the backward
        twice: dQ and dK/dV kernels).  No ratio is a pass mark.

    python tools/attention_mask_bench.py --unmasked-only --label NAME
        one process's series of the UNMASKED path only, for alternating-process comparisons of two libraries (BDETR_LIB selects
        the library; the Python code is the same).

A measurement path that finds no GPU fails."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from boosted_detr_amd import kernels as k  # noqa: E402

B, H, D = 16, 8, 256
SHAPES = (("encoder self", 400, 400), ("decoder cross", 100, 400))
HBM_BYTES_PER_S = 6.3e12          # achievable streaming rate of an MI355X (8 TB/s peak)
WARMUP, WINDOWS, CALLS = 5, 20, 20
SCALE = 32 ** -0.5


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS * 1e3      # us per call


def fmt(ws):
    return "%8.1f us  (%.1f - %.1f)" % (statistics.median(ws), min(ws), max(ws))


def variants(nq, nk, g, only_unmasked):
    out = [("unmasked", None)]
    if only_unmasked:
        return out
    key_f = torch.rand(B, 1, 1, nk, device="cuda", generator=g) * 2 - 0.5
    full_f = torch.rand(B, H, nq, nk, device="cuda", generator=g) * 2 - 0.5
    out += [("key-only f32 [B,1,1,k]", key_f), ("key-only bool [B,1,1,k]", key_f > 0.25),
            ("full f32 [B,h,q,k]", full_f), ("full bool [B,h,q,k]", full_f > 0.25)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--unmasked-only", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing measured")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device="cuda").manual_seed(0)
    if not a.unmasked_only:
        say("attention core with a mask - tools/attention_mask_bench.py; device: %s" % torch.cuda.get_device_name(0))
        say("B = %d, h = %d, head dim 32, policy 'split'; per variant %d warm-up calls, then %d windows of %d calls (device events),"
            % (B, H, WARMUP, WINDOWS, CALLS))
        say("the variants interleaved window by window in one process; median (min - max) per call.  'mask bytes at HBM rate': the")
        say("mask's own bytes over %.1f TB/s, once for the forward and twice for the backward (dQ and dK/dV kernels each read it)."
            % (HBM_BYTES_PER_S / 1e12))
        say("No ratio is a pass mark; the masked kernels read each mask element with a scalar load of its own.")
    with k.gemm_precision("split"):
        for name, nq, nk in SHAPES:
            q, kk, v = (torch.randn(B, n, D, device="cuda", generator=g) for n in (nq, nk, nk))
            do = torch.randn(B, H, nq, 32, device="cuda", generator=g)
            cases = []
            for label, m in variants(nq, nk, g, a.unmasked_only):
                kw = {} if m is None else {"mask": m}
                o, lse = k.attention_fwd(q, kk, v, H, SCALE, **kw)
                fwd = (lambda kw=kw: k.attention_fwd(q, kk, v, H, SCALE, **kw))
                bwd = (lambda kw=kw, o=o, lse=lse: k.attention_bwd(q, kk, v, o, do, lse, H, SCALE, **kw))
                for _ in range(WARMUP):
                    fwd(), bwd()
                cases.append((label, m, fwd, bwd, [], []))
            torch.cuda.synchronize()
            for _ in range(WINDOWS):
                for _, _, fwd, bwd, wf, wb in cases:
                    wf.append(window(fwd))
                    wb.append(window(bwd))
            if a.unmasked_only:
                _, _, _, _, wf, wb = cases[0]
                say("  %-10s %-13s %dx%d  fwd %s   bwd %s" % (a.label, name, nq, nk, fmt(wf), fmt(wb)))
                continue
            say()
            say("%s, %d x %d" % (name, nq, nk))
            for label, m, _, _, wf, wb in cases:
                extra = ""
                if m is not None:
                    nbytes = m.numel() * m.element_size()
                    extra = "   mask %9.3f MB = %6.2f us at HBM rate (fwd), %6.2f us (bwd)" % (
                        nbytes / 1e6, nbytes / HBM_BYTES_PER_S * 1e6, 2 * nbytes / HBM_BYTES_PER_S * 1e6)
                say("  %-24s fwd %s   bwd %s%s" % (label, fmt(wf), fmt(wb), extra))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
