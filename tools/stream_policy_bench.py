"""Isolated timing of every kernel that takes a cache-policy template parameter (csrc/stream.h), policy off against on.

The library reads BDETR_STREAM_POLICY once per process, so this tool runs itself once per policy value as a child process and
prints both columns side by side.  Rows: the kernel at the four ResNet stage shapes of bench.py configs[1] (batch 16, 640 x 640),
each twice - "hot": one operand set, launched back to back (the 256 MiB Infinity Cache holds whatever fits from the launch before);
"cold": as many operand sets as it takes to exceed 512 MiB, used round-robin, so that no launch finds its operands cached.  The
cold rows are the ones that resemble the training step, where tens of GB pass between two uses of a tensor.

    python tools/stream_policy_bench.py [--policies 0,63] [--iters 20]

What wins here does not decide the library's default: the step does (profiles/README.md)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MARK = "STREAM_POLICY_BENCH "
STAGES = [(16, 160, 256), (16, 80, 512), (16, 40, 1024), (16, 20, 2048)]      # N, H = W, C of a stage's output
COLD_BYTES = 512 << 20


def child(iters):
    import torch
    from boosted_detr_amd import _lib
    from boosted_detr_amd import kernels as k
    rows_out = []

    def timed(name, make, run, nbytes):
        """make() -> one operand set; run(set).  Hot: one set; cold: enough sets for COLD_BYTES, round-robin."""
        for mode in ("hot", "cold"):
            nsets = 1 if mode == "hot" else max(2, -(-COLD_BYTES // nbytes))
            sets = [make() for _ in range(nsets)]
            for s in sets[:2]:
                run(s)
            torch.cuda.synchronize()
            n = max(iters, nsets)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(n):
                run(sets[i % nsets])
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / n
            rows_out.append({"name": "%s %s" % (name, mode), "us": us, "GBps": nbytes / us * 1e-3})
            del sets
            torch.cuda.empty_cache()

    rnd = lambda *s: torch.randn(*s, device="cuda")
    for N, H, C in STAGES:
        rows = N * H * H
        T = rows * C * 4
        par = [torch.rand(C, device="cuda") + 0.5 for _ in range(4)]
        mean, rstd, gamma, beta = par
        tag = "%dx%dx%dx%d" % (N, H, H, C)
        Cm = C // 4                                                # a unit's inner width

        def make_apply():
            x, r = rnd(rows, C), rnd(rows, C)
            return x, k.bn_apply_p16(r, *par, None, True, want_fp32=False, want_bf16=False)[1]
        timed("bn_apply_p16 +res f16 -> f16+bits " + tag, make_apply,
              lambda s: k.bn_apply_p16(s[0], *par, s[1], True, want_fp32=False, want_bf16=False, residual_p16=True, want_mask=True), 3 * T + T // 32)
        pm = [p[:Cm].contiguous() for p in par]
        timed("bn_apply_p16 plain -> f16+bf16 %dx%d" % (rows, Cm), lambda: (rnd(rows, Cm),),
              lambda s: k.bn_apply_p16(s[0], *pm, None, True, want_fp32=False), 3 * T // 4)
        timed("bn_apply_p16 even pixels " + tag, make_apply,
              lambda s: k.bn_apply_p16(s[0], *par, s[1], True, want_fp32=False, want_bf16=False, residual_p16=True, want_mask=True, even_pixels=(H, H)), (3 * T + T // 32) // 4)

        def make_bwd():
            x, dy = rnd(rows, C), rnd(rows, C)
            bits = k.bn_apply_p16(x, *par, None, True, want_fp32=False, want_bf16=False, want_mask=True)[3]      # (the library wants one tensor output)
            pre = (rnd(64, C), rnd(64, C), 64)
            return x, dy, bits, pre
        timed("bn_bwd_p16 reduce+apply bit mask " + tag, make_bwd,
              lambda s: k.bn_bwd_p16(s[1], s[2], s[0], mean, rstd, gamma, True, False, beta=beta, out_p16=2), 5 * T + T // 16)
        timed("bn_bwd_p16 apply only (pre sums) " + tag, make_bwd,
              lambda s: k.bn_bwd_p16(s[1], s[2], s[0], mean, rstd, gamma, True, False, beta=beta, out_p16=2, pre=s[3]), 3 * T + T // 32)
        timed("bn_bwd_p16 recompute %dx%d" % (rows, Cm), lambda: (rnd(rows, Cm), rnd(rows, Cm)),
              lambda s: k.bn_bwd_p16(s[1], None, s[0], pm[0], pm[1], pm[2], True, False, beta=pm[3]), 5 * T // 4)
        timed("colstats %dx%d" % (rows, Cm), lambda: (rnd(rows, Cm),), lambda s: k.colstats(s[0]), T // 4)
        timed("relu_mask_apply " + tag, make_bwd, lambda s: k.relu_mask_apply_(s[1], s[2]), 2 * T + T // 32)

        # the fused 1x1 backward-data of a unit's first convolution: dy [rows, C/4] -> dx [rows, C] += old * mask, + the previous unit's sums
        g = k.ConvGeom(N, H, H, C, Cm, 1, 1, 1, 0)
        _, wt = k.p16_pack_conv_weights(rnd(Cm, 1, 1, C) * C ** -0.5, want_fwd=False)

        def make_acc():
            x, dy, bits, _ = make_bwd()
            _, dyb = k.p16_pack(rnd(rows, Cm), want_f16=False)
            return dyb, dy, bits, (x, mean, rstd, gamma, beta, bits)
        timed("bwd-data masked accumulate + sums " + tag, make_acc,
              lambda s: k.p16_conv2d_bwd_data_masked_accum(s[0], wt, g, s[1].view(N, H, H, C), s[2], bn_ctx=s[3]), 3 * T + T // 4 + T // 16)

    # the stem pair: raw conv output [16, 320, 320, 64]
    N, H, C = 16, 320, 64
    par = [torch.rand(C, device="cuda") + 0.5 for _ in range(4)]
    T = N * H * H * C * 4
    timed("stem_pool_fwd 16x320x320x64", lambda: (rnd(N, H, H, C),), lambda s: k.stem_pool_fwd(s[0], *par), T + T // 4 + T // 16)

    def make_stem():
        y = rnd(N, H, H, C)
        _, _, tap = k.stem_pool_fwd(y, *par)
        return y, tap, rnd(N, H // 2, H // 2, C)
    timed("stem_pool_bwd (reduce + apply) 16x320x320x64", make_stem, lambda s: k.stem_pool_bwd(s[2], s[1], s[0], *par, dy_p16=True), 3 * T + T // 2)

    # optimizer step and weight pack on ResNet-50-sized tensors (23.5 M conv weights in 53 tensors' worth of the widest shapes)
    from boosted_detr_amd.engine import Variable
    from boosted_detr_amd.training import SGD
    shapes = [(512, 3, 3, 512)] * 3 + [(2048, 1, 1, 512)] * 3 + [(512, 1, 1, 2048)] * 3 + [(256, 3, 3, 256)] * 6 + [(1024, 1, 1, 256)] * 6 + [(256, 1, 1, 1024)] * 6
    vs = []
    for i, s in enumerate(shapes):
        numel = s[0] * s[1] * s[2] * s[3]
        v = Variable("bench/t%d" % i, (numel,))
        v.value = 0.05 * rnd(numel)
        vs.append(v)
    opt = SGD(1e-3, momentum=0.9, nesterov=True, clipnorm=0.1)
    opt.build(vs)
    opt.flat_grad.copy_(1e-3 * rnd(opt.flat_grad.numel()))
    n = sum(v.value.numel() for v in vs)
    timed("sgd_nesterov_clipnorm %.1f M elements" % (n * 1e-6), lambda: None, lambda s: opt.apply_gradients(), 24 * n)
    wf = [torch.empty_like(v.value) for v in vs]
    wtt = [torch.empty(s[3], s[1], s[2], s[0], device="cuda") for s in shapes]
    table = torch.tensor([[v.value.data_ptr(), f.data_ptr(), t.data_ptr(), *s] for v, f, t, s in zip(vs, wf, wtt, shapes)], dtype=torch.int64, device="cuda")
    timed("p16_pack_conv_weights_multi %.1f M elements" % (n * 1e-6), lambda: None, lambda s: k.p16_pack_conv_weights_multi(table), 16 * n)
    print(MARK + json.dumps({"policy": int(_lib.lib().bdetr_stream_policy()), "rows": rows_out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", default="0,63", help="comma-separated BDETR_STREAM_POLICY values, one child process each")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.iters)
    cols = {}
    for p in [int(v) for v in a.policies.split(",")]:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(a.iters)], env=dict(os.environ, BDETR_STREAM_POLICY=str(p)),
                           capture_output=True, text=True, timeout=900)          # (a hung child ends the tool)
        if r.returncode != 0:
            sys.exit("policy %d: child failed\n%s\n%s" % (p, r.stdout[-2000:], r.stderr[-4000:]))
        out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith(MARK)][0][len(MARK):])
        assert out["policy"] == p
        cols[p] = out["rows"]
    ps = list(cols)
    print("%-62s" % "kernel (us per launch | GB/s)" + "".join("   policy %-3d         " % p for p in ps) + ("  on/off" if len(ps) == 2 else ""))
    for i, row in enumerate(cols[ps[0]]):
        line = "%-62s" % row["name"] + "".join("  %9.1f us %6.0f  " % (cols[p][i]["us"], cols[p][i]["GBps"]) for p in ps)
        if len(ps) == 2:
            line += "  %.3f" % (cols[ps[1]][i]["us"] / row["us"])
        print(line, flush=True)


if __name__ == "__main__":
    main()
