"""Child process of tests/test_variants_gpu.py: runs one named list of kernel cases under whatever variant switches the
parent put into the environment (the choosers read them once per process) and prints one JSON line.

    python tests/_variant_child.py <case-list-name>

Per case the line holds, for every product the case compared with its fp64 reference, max|got - ref| / max|ref| with the
bar it was held to and the index of the worst element ((n, h, w, channel) for the NHWC products), and the set of
(kind, bm, bn) tuples the profiling hooks of the conv/GEMM family recorded while the case ran (the encoding
tests/test_precision_gpu.py::_prof_tuples reads).  A failed comparison is recorded and the next case runs; any other error
ends the child with a traceback.

Every case runs inside a guard arena (tests/_guard.py): its operands, results and workspaces sit between 0xFF margins, and the
report's "guard" is null or what the arena found - a changed margin, a changed read-only operand, an unguarded result or a NaN
left in a result.  (One run per case: the two-fill comparison of integer results belongs to tests/test_memory_bounds_gpu.py.)

The module is also imported by the parent (no GPU work at import time) for the case lists and what each case must launch."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MARK = "VARIANT_JSON "
AR_F16, AR_BF16 = 3, 4                      # csrc/gemm_common.h: AR_P16_F16 (forward), AR_P16_BF16 (gradients)
# BDETR_HCONV_TILE -> (BM, BN, widest W the halo buffer admits: BM + 2 W + 2 <= halo_cap(BN), csrc/hconv.hip)
HCONV_TILES = {"256128": (256, 128, 91), "128128": (128, 128, 155), "256064": (256, 64, 127)}
STILES = {"128x128": (128, 128), "128x64": (128, 64), "64x64": (64, 64)}


def hconv_tuple(tile, fwd):
    bm, bn, _ = HCONV_TILES[tile]
    return ((AR_F16 if fwd else AR_BF16) * 10000 + 4000, bm, bn * 10 + 3)


def hconv_admits(tile, W, cin, J):
    """The admission rule of a forced tile, restated from the issue that introduced these tests - NOT read from the library."""
    bm, bn, cap = HCONV_TILES[tile]
    return cin % 32 == 0 and J % bn == 0 and W <= cap


def hconv_cases(tile):
    """3x3 / stride 1 / pad 1 geometries for one forced tile of the halo-resident kernel: [("p16", (N, H, W, C, K, 3, 1, 1), what)]."""
    bm, bn, cap = HCONV_TILES[tile]
    cb = bn                                                     # C = K = one column tile
    out = [("p16", (2, 3, cap, cb, cb, 3, 1, 1), "W at the halo cap"),
           ("p16", (2, 3, cap + 1, cb, cb, 3, 1, 1), "one past the cap")]
    for nhw in ((1, 1, 1), (3, 1, 7), (3, 7, 1), (5, 3, 3)):
        out.append(("p16", nhw + (cb, cb, 3, 1, 1), "degenerate images"))
    for nhw in ((1, 257, 1), (1, 17, 15), (1, 3, 43), (1, 127, 1)):            # rows = 257, 255, 129, 127
        out.append(("p16", nhw + (cb, cb, 3, 1, 1), "ragged last tile"))
    for nhw in ((3, 9, 11), (7, 13, 5)):
        out.append(("p16", nhw + (cb, cb, 3, 1, 1), "image boundary inside a tile"))
    jb = 128 if bn == 128 else 64
    for cin in (32, 96):                                        # the reduction runs over C forward and over K backward
        out.append(("p16", (3, 9, 11, cin, jb, 3, 1, 1), "%d chunk(s) forward" % (cin // 32)))
        out.append(("p16", (3, 9, 11, jb, cin, 3, 1, 1), "%d chunk(s) backward" % (cin // 32)))
    if bn == 64:
        out.append(("p16", (3, 9, 11, 96, 192, 3, 1, 1), "3 chunks forward, 3 column tiles"))
    jw = 384 if bn == 128 else 192
    out.append(("p16", (3, 9, 11, jw, jw, 3, 1, 1), "several column tiles"))
    out.append(("bnstats", (3, 9, 11, cb, cb, 3), "fused BatchNorm-backward sums, rows % BM != 0"))
    return out


def stile_cases(tile):
    """Fused backward-data epilogues on one forced sgemm tile (BDETR_HCONV=0): rows = 297, C % BN != 0; K = 520 keeps the
    forced 128x128 tile on the dense float4 epilogue (bwd_data_plan() halves it for K <= 512)."""
    return [("bnstats", (3, 9, 11, 160, 64, 3), "3x3 fused sums"), ("bnstats", (3, 9, 11, 136, 520, 1), "1x1 fused sums"),
            ("masked", (3, 9, 11, 136, 520, False), "masked accumulate"), ("masked", (3, 9, 11, 136, 520, True), "masked accumulate + fused sums")]


def _p16_rows(pred):
    from test_p16_gpu import P16_CONVS
    return [s for s in P16_CONVS if pred(s)]


def wgrad_cases():
    return [("p16", s, "") for s in _p16_rows(lambda s: s[5] == 1)]


TILE_LINEARS = [(300, 256, 256), (130, 52, 48), (1600, 1024, 82)]                                  # the ragged rows of test_precision_gpu.LINEARS / CONVS
TILE_CONVS = [(2, 20, 20, 256, 128, 1, 2, 0), (1, 9, 11, 128, 32, 3, 1, 1), (3, 7, 7, 512, 2048, 1, 1, 0)]
ATTN_SHAPES = [(2, 8, 400, 400), (2, 8, 100, 400), (3, 8, 100, 100), (2, 8, 49, 49), (1, 4, 50, 49), (1, 8, 300, 1050)]


def tile_cases():
    return [(kind, (mode,) + s, "") for mode in ("fp32", "split") for kind, rows in (("linear", TILE_LINEARS), ("conv", TILE_CONVS)) for s in rows]


def case_list(name):
    head, _, arg = name.partition(":")
    if head == "hconv":
        return hconv_cases(arg)
    if head == "stile":
        return stile_cases(arg)
    return {"wgrad": wgrad_cases, "tile": tile_cases, "attn": lambda: [("attn", s, "") for s in ATTN_SHAPES]}[head]()


# ---------------------------------------------------------------------------------------------- the child itself
RECORDS = []
P16_PRODUCTS = ["fwd", "stat_sum", "stat_sq", "bwd_data", "bwd_data_accum", "bwd_weight", "bwd_weight_xf16", "bwd_weight_det", "bwd_weight_det_accum"]


def _install_recording_close():
    """Wrap the suite's `close` so that every comparison of the imported case bodies also leaves its figure behind."""
    import numpy as np
    import test_kernels_gpu
    import test_p16_gpu
    import test_precision_gpu
    plain = test_kernels_gpu.close

    def close(got, want, rtol=2e-5, atol=None):
        g, w = got.detach().cpu().double(), want.detach().cpu().double()
        at = None
        if g.shape == w.shape and g.numel():
            d = (g - w).abs()
            at = [int(i) for i in np.unravel_index(int(d.argmax()), tuple(d.shape))]
            RECORDS.append({"rtol": rtol, "rel": d.max().item() / (w.abs().max().item() + 1e-30), "at": at})
        try:
            plain(got, want, rtol=rtol, atol=atol)
        except AssertionError as e:
            raise AssertionError("%s; worst element at %s of %s" % (e, at, tuple(g.shape))) from None

    test_p16_gpu.close = test_precision_gpu.close = close
    return close


def _conv_dx64(dy, w, R):
    """fp64 input gradient of the stride-1 'same' convolution: dy [N,H,W,K], w [K,R,R,C] -> [N,H,W,C]."""
    import torch
    import torch.nn.functional as F
    N, H, W, _ = dy.shape
    x0 = torch.zeros(N, w.shape[3], H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x0, w.double().permute(0, 3, 1, 2), padding=R // 2).backward(dy.double().permute(0, 3, 1, 2))
    return x0.grad.permute(0, 2, 3, 1).reshape(N * H * W, -1)


class _Unit:
    """A BatchNorm(+ shortcut)+ReLU layer with host-chosen parameters whose fp64 pre-activation keeps 1e-4 clear of zero, so
    that the fp32 kernels and the fp64 reference take the same ReLU decision for every element."""

    def __init__(self, rows, C, seed, shortcut):
        import torch
        from test_kernels_gpu import rnd
        self.gamma, self.beta = 1 + 0.1 * rnd(C, seed=seed + 1), 0.1 * rnd(C, seed=seed + 2)
        self.mean, self.rstd = 0.3 + 0.1 * rnd(C, seed=seed + 3), 0.5 + 0.05 * rnd(C, seed=seed + 4).abs()
        self.shortcut = rnd(rows, C, seed=seed + 5) if shortcut else None
        y = rnd(rows, C, seed=seed) * 2 + 0.3
        gen = torch.Generator().manual_seed(seed + 6)
        for _ in range(8):                                      # resample (on the host) the elements the margin excludes
            bad = self.pre64(y).abs() < 1e-4
            if not bad.any():
                break
            y[bad] = torch.randn(int(bad.sum()), generator=gen) * 2 + 0.3
        self.y = y
        excluded = int((self.pre64(y).abs() < 1e-4).sum())
        assert excluded == 0, "ReLU margin: %d pre-activations within 1e-4 of zero" % excluded       # a condition on the inputs, not a tolerance
        self.on = (self.pre64(y) > 0).double()
        self.xhat = (y.double() - self.mean.double()) * self.rstd.double()

    def pre64(self, y):
        p = (y.double() - self.mean.double()) * (self.rstd.double() * self.gamma.double()) + self.beta.double()
        return p if self.shortcut is None else p + self.shortcut.double()

    def device(self):
        from test_kernels_gpu import dev
        return tuple(dev(t) for t in (self.y, self.mean, self.rstd, self.gamma, self.beta))

    def bits(self):
        from boosted_detr_amd import kernels as k
        from test_kernels_gpu import dev
        return k.bn_apply_p16(*self.device(), dev(self.shortcut), True, want_fp32=False, want_f16=True, want_bf16=False, want_mask=True)[3]


def bnstats_case(close, N, H, W, C, K, R):
    """bdetr_p16_conv2d_bwd_data_bnstats: dx bit-identical to the plain launch and within 6e-5 of fp64; bn_bwd_p16 fed with the
    partial rows agrees with its own two-pass reduction (1e-5) AND with the fp64 sums dbeta = sum(g), dgamma = sum(g * xhat),
    g = dx * [fp64 pre-activation > 0] (1e-4 x max, the bar of the forward statistics)."""
    import torch
    from boosted_detr_amd import kernels as k
    from test_kernels_gpu import dev, rnd
    g = k.ConvGeom(N, H, W, C, K, R, R, 1, R // 2)
    rows = N * H * W
    u = _Unit(rows, C, 1, shortcut=False)
    y, mean, rstd, gamma, beta = u.device()
    w, dy = rnd(K, R, R, C, seed=4, scale=(R * R * C) ** -0.5), rnd(N, H, W, K, seed=5)
    _, wt = k.p16_pack_conv_weights(dev(w), want_fwd=False)
    _, dyb = k.p16_pack(dev(dy), want_f16=False)
    dx_plain = k.p16_conv2d_bwd_data(dyb, wt, g)
    dx, parts = k.p16_conv2d_bwd_data_bnstats(dyb, wt, g, y, mean, rstd, gamma, beta, True)
    assert torch.equal(dx, dx_plain)
    dx64 = _conv_dx64(dy, w, R)
    close(dx.view(rows, C), dx64, rtol=6e-5)
    ref = k.bn_bwd_p16(dx.view(rows, C), None, y, mean, rstd, gamma, True, False, beta=beta, want_fp32=True)
    got = k.bn_bwd_p16(dx.view(rows, C), None, y, mean, rstd, gamma, True, False, beta=beta, want_fp32=True, pre=parts)
    close(got[2], ref[2], rtol=1e-5); close(got[3], ref[3], rtol=1e-5); close(got[1], ref[1], rtol=1e-5)
    g64 = dx64 * u.on
    close(parts[0][:parts[2]].sum(0), g64.sum(0), rtol=1e-4); close(parts[1][:parts[2]].sum(0), (g64 * u.xhat).sum(0), rtol=1e-4)
    close(got[3], g64.sum(0), rtol=1e-4); close(got[2], (g64 * u.xhat).sum(0), rtol=1e-4)


def masked_case(close, N, H, W, C, K, with_ctx):
    """bdetr_p16_conv2d_bwd_data_masked_accum (1x1): product + old * mask against fp64 (6e-5), the mask being the fp64 ReLU decision
    of this unit; with a BatchNorm context: dx bit-identical to the plain masked accumulate, the partial rows agree with
    bn_bwd_p16's own reduction (1e-5) and with the fp64 sums under the previous unit's fp64 ReLU decision (1e-4 x max)."""
    import torch
    from boosted_detr_amd import kernels as k
    from test_kernels_gpu import dev, rnd
    g = k.ConvGeom(N, H, W, C, K, 1, 1, 1, 0)
    rows = N * H * W
    prev, this = _Unit(rows, C, 10, shortcut=True), _Unit(rows, C, 20, shortcut=True)
    d_out, w, dy = rnd(N, H, W, C, seed=5), rnd(K, 1, 1, C, seed=6, scale=C ** -0.5), rnd(N, H, W, K, seed=7)
    _, wt = k.p16_pack_conv_weights(dev(w), want_fwd=False)
    _, dyb = k.p16_pack(dev(dy), want_f16=False)
    bits_this = this.bits()
    plain = k.p16_conv2d_bwd_data_masked_accum(dyb, wt, g, dev(d_out), bits_this)
    want = dy.double().reshape(rows, K) @ w.double().reshape(K, C) + d_out.double().reshape(rows, C) * this.on
    close(plain.view(rows, C), want, rtol=6e-5)
    if not with_ctx:
        return
    y, mean, rstd, gamma, beta = prev.device()
    bits_prev = prev.bits()
    dx, parts = k.p16_conv2d_bwd_data_masked_accum(dyb, wt, g, dev(d_out), bits_this, bn_ctx=(y, mean, rstd, gamma, beta, bits_prev))
    assert torch.equal(dx, plain)
    ref = k.bn_bwd_p16(dx.view(rows, C), bits_prev, y, mean, rstd, gamma, True, False, beta=beta, want_fp32=True, out_p16=2)
    got = k.bn_bwd_p16(dx.view(rows, C), bits_prev, y, mean, rstd, gamma, True, False, beta=beta, want_fp32=True, out_p16=2, pre=parts)
    close(got[2], ref[2], rtol=1e-5); close(got[3], ref[3], rtol=1e-5); close(got[1], ref[1], rtol=1e-5)
    g64 = want * prev.on
    close(parts[0][:parts[2]].sum(0), g64.sum(0), rtol=1e-4); close(parts[1][:parts[2]].sum(0), (g64 * prev.xhat).sum(0), rtol=1e-4)
    close(got[3], g64.sum(0), rtol=1e-4); close(got[2], (g64 * prev.xhat).sum(0), rtol=1e-4)


def attn_case(close, B, h, nq, nk):
    """The inputs and fp64 reference of test_kernels_gpu.test_fused_attention_fwd_bwd under policy 'split', held to the bars of
    policy 'fp32' (1e-5 forward, 5e-5 gradients): with BDETR_ATTN_SPLIT=0 every attention product runs the exact-fp32 MFMA."""
    import numpy as np
    import torch
    from boosted_detr_amd import kernels as k
    from test_kernels_gpu import dev, rnd
    D = h * 32
    Q, Kt, V = rnd(B, nq, D, seed=1), rnd(B, nk, D, seed=2), rnd(B, nk, D, seed=3)
    Q[0, 0] *= 6.0
    dO = rnd(B, h, nq, 32, seed=4)
    scale = 1.0 / np.sqrt(32.0)
    with k.gemm_precision("split"):
        o, lse = k.attention_fwd(dev(Q), dev(Kt), dev(V), h, scale)
    Qd, Kd, Vd = (t.double().requires_grad_(True) for t in (Q, Kt, V))
    s = (Qd.view(B, nq, h, 32).permute(0, 2, 1, 3) @ Kd.view(B, nk, h, 32).permute(0, 2, 3, 1)) * scale
    ref = torch.softmax(s, -1) @ Vd.view(B, nk, h, 32).permute(0, 2, 1, 3)
    close(o, ref, rtol=1e-5); close(lse, torch.logsumexp(s, -1), rtol=1e-5)
    ref.backward(dO.double())
    with k.gemm_precision("split"):
        dq, dk, dv = k.attention_bwd(dev(Q), dev(Kt), dev(V), o, dev(dO), lse, h, scale)
    close(dq, Qd.grad, rtol=5e-5); close(dk, Kd.grad, rtol=5e-5); close(dv, Vd.grad, rtol=5e-5)


def main(name):
    import tempfile
    import torch
    import _guard
    from boosted_detr_amd import _lib
    from boosted_detr_amd import kernels as k
    from test_p16_gpu import p16_conv_case
    from test_precision_gpu import _prof_tuples, conv_case, linear_case
    assert torch.cuda.is_available(), "the variant child needs a GPU"
    close = _install_recording_close()
    L = _lib.lib()

    def policy_case(fn):
        def run(mode, *shape):
            with k.gemm_precision(mode):
                fn(mode, *shape)
        return run

    bodies = {"p16": p16_conv_case, "bnstats": lambda *a: bnstats_case(close, *a), "masked": lambda *a: masked_case(close, *a),
              "attn": lambda *a: attn_case(close, *a), "linear": policy_case(linear_case), "conv": policy_case(conv_case)}
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        for kind, args, what in case_list(name):
            del RECORDS[:]
            failed = guard = None
            arena = _guard.Arena("cuda")
            L.bdetr_prof_enable(1)
            try:
                with arena.armed():
                    bodies[kind](*args)
            except AssertionError as e:
                failed = str(e)[:600] or "assertion failed"
            finally:
                tuples = sorted(_prof_tuples(os.path.join(tmp, "prof.csv")))
                L.bdetr_prof_enable(0)
            try:
                arena.verify()
            except _guard.GuardError as e:
                guard = str(e)[:1500]
            del arena
            names = P16_PRODUCTS if kind == "p16" and len(RECORDS) == len(P16_PRODUCTS) else ["p%d" % i for i in range(len(RECORDS))]
            results.append({"case": [kind] + list(args), "what": what, "failed": failed, "guard": guard, "tuples": [list(t) for t in tuples],
                            "errors": {n: r for n, r in zip(names, RECORDS)}})
    print(MARK + json.dumps({"list": name, "cases": results}), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
