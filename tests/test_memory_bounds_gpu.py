"""Every training-path kernel family inside the guard arena (tests/_guard.py): operands, results and workspaces sit between
0xFF margins the test owns, fresh results start as NaN (integers: two runs, 0xFF and 0x5A).  A store past an output, a load
past an input that reaches the result, an element nobody wrote and a scribble on a read-only operand each fail the case.

The case bodies are the suite's own (imported and called as plain functions) wherever they build every operand with `dev`;
where an existing body allocates a destination with torch directly, the body here restates it with `dev` / `kernels.empty` and
keeps the reference and the tolerance.  The shapes are the smallest with a ragged edge in every tile dimension - not the
workload's.  `run_guarded` asserts the four conditions of _guard.verify after the body's own comparisons pass."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _guard
import test_aux_losses_gpu
import test_kernels_gpu
import test_matcher_gpu
import test_panoptic_gpu  # noqa: F401  (imported so that its `dev` is rebound too)
import test_panoptic_train_gpu
import test_p16_gpu
import test_precision_gpu
import test_rowchain_gpu
import test_stem_gpu
from test_kernels_gpu import close, dev, rnd

pytestmark = pytest.mark.gpu

# forward / gradient bars per policy: tests/test_precision_gpu.py TOL_FWD / TOL, and 'mixed' = exact-fp32 forward with split-bf16
# gradient products (kernels.set_gemm_precision), i.e. the fp32 forward bar and the split gradient bar
TOL_FWD = dict(test_precision_gpu.TOL_FWD, mixed=test_precision_gpu.TOL_FWD["fp32"])
TOL = dict(test_precision_gpu.TOL, mixed=test_precision_gpu.TOL["split"])
POLICIES = ["fp32", "mixed", "split", "bf16x3"]


def guarded(cuda, body, *args, **kw):
    assert _guard.run_guarded(cuda, body, *args, **kw) >= 1


def arena():
    return _guard.ACTIVE[-1]


# ------------------------------------------------------------------------------------------------------------ dense GEMM
def linear_body(mode, M, K, O):
    from boosted_detr_amd import kernels as k
    x, w, b, dy = rnd(M, K, seed=1), rnd(O, K, seed=2, scale=K ** -0.5), rnd(O, seed=3), rnd(M, O, seed=4)
    base = rnd(M, K, seed=5)
    with k.gemm_precision(mode):
        for det in (False, True):                       # deterministic: the split-K slabs are a workspace of their own, guarded like the rest
            prev = k.set_deterministic(det)
            try:
                close(k.linear_fwd(dev(x), dev(w), dev(b), 1), (x.double() @ w.double().T + b.double()).relu(), rtol=TOL_FWD[mode])
                close(k.linear_fwd(dev(x), dev(w), None, 0), x.double() @ w.double().T, rtol=TOL_FWD[mode])
                close(k.linear_bwd_data(dev(dy), dev(w)), dy.double() @ w.double(), rtol=TOL[mode])
                dx = dev(base)
                k.linear_bwd_data(dev(dy), dev(w), dx=dx, accumulate=True)
                close(dx, base.double() + dy.double() @ w.double(), rtol=TOL[mode])
                close(k.linear_bwd_weight(dev(dy), dev(x)), dy.double().T @ x.double(), rtol=TOL[mode])
                dw = dev(torch.zeros(O, K))
                k.linear_bwd_weight(dev(dy), dev(x), dw=dw, prezeroed=True)
                close(dw, dy.double().T @ x.double(), rtol=TOL[mode])
            finally:
                k.set_deterministic(prev)


@pytest.mark.parametrize("mode", POLICIES)
@pytest.mark.parametrize("M,K,O", [(1, 32, 4), (63, 36, 4), (65, 32, 82), (130, 50, 48), (257, 260, 132)])
def test_dense_gemm(cuda, M, K, O, mode):
    guarded(cuda, linear_body, mode, M, K, O)


def long_reduction_body():
    """A weight gradient whose reduction is long enough for _auto_splitk to split it (M // 128 > 1): atomics, and slabs + fold."""
    from boosted_detr_amd import kernels as k
    M, K, O = 515, 36, 20
    x, dy = rnd(M, K, seed=1), rnd(M, O, seed=4)
    assert k._auto_splitk(O, K, M) > 1
    for det in (False, True):
        prev = k.set_deterministic(det)
        try:
            close(k.linear_bwd_weight(dev(dy), dev(x)), dy.double().T @ x.double(), rtol=TOL["mixed"])
        finally:
            k.set_deterministic(prev)


def test_dense_gemm_split_k(cuda):
    guarded(cuda, long_reduction_body)


def batched_body():
    """test_kernels_gpu.test_gemm_batched_attention_shapes at one shape, the destinations fresh (NaN) guarded tensors."""
    from boosted_detr_amd import kernels as k
    B, h, q, kk, d = 2, 4, 50, 49, 32
    D = h * d
    Q, Kt, V = rnd(B, q, D, seed=1), rnd(B, kk, D, seed=2), rnd(B, kk, D, seed=3)
    like = dev(Q)
    s = k.empty(B, h, q, kk, like=like)
    k.gemm_raw(q, kk, d, like, D, True, dev(Kt), D, True, s, kk, nb0=B, nb1=h, sa=(q * D, d), sb=(kk * D, d), sc=(h * q * kk, q * kk), alpha=0.25)
    Qh = Q.view(B, q, h, d).permute(0, 2, 1, 3).double()
    Kh = Kt.view(B, kk, h, d).permute(0, 2, 1, 3).double()
    Vh = V.view(B, kk, h, d).permute(0, 2, 1, 3).double()
    ref = 0.25 * Qh @ Kh.transpose(-1, -2)
    close(s, ref)
    p = torch.softmax(ref, -1).float()
    o = k.empty(B, h, q, d, like=like)
    k.gemm_raw(q, d, kk, dev(p), kk, True, dev(V), D, False, o, d, nb0=B, nb1=h, sa=(h * q * kk, q * kk), sb=(kk * D, d), sc=(h * q * d, q * d))
    close(o, p.double() @ Vh)
    dO = rnd(B, h, q, d, seed=4)
    dV = k.empty(B, kk, D, like=like)
    k.gemm_raw(kk, d, q, dev(p), kk, False, dev(dO), d, False, dV, D, nb0=B, nb1=h, sa=(h * q * kk, q * kk), sb=(h * q * d, q * d), sc=(kk * D, d))
    close(dV, (p.double().transpose(-1, -2) @ dO.double()).permute(0, 2, 1, 3).reshape(B, kk, D))


def test_gemm_batched(cuda):
    guarded(cuda, batched_body)


def grouped_body(mode):
    from boosted_detr_amd import kernels as k
    rows, K, O = (1, 65, 130), 52, 48
    xs = [rnd(m, K, seed=10 + m) for m in rows]
    ws = [rnd(O, K, seed=20 + i, scale=K ** -0.5) for i in range(3)]
    bs = [rnd(O, seed=30 + i) for i in range(3)]
    dys = [rnd(m, O, seed=40 + m) for m in rows]
    with k.gemm_precision(mode):
        ys = k.linear_fwd_group([dev(x) for x in xs], [dev(w) for w in ws], [dev(b) for b in bs])
        for y, x, w, b in zip(ys, xs, ws, bs):
            close(y, x.double() @ w.double().T + b.double(), rtol=TOL_FWD[mode])
        dxs = k.linear_bwd_data_group([dev(d) for d in dys], [dev(w) for w in ws])
        for dx, dy, w in zip(dxs, dys, ws):
            close(dx, dy.double() @ w.double(), rtol=TOL[mode])
        # ragged members: one launch each; then three members of one shape: ONE grouped launch.  Destinations: fresh, zeroed, zeroed
        for members in (rows, (130, 130, 130)):
            dys_, xs_ = [rnd(m, O, seed=50 + i) for i, m in enumerate(members)], [rnd(m, K, seed=60 + i) for i, m in enumerate(members)]
            dws = [k.empty(O, K, like=dev(bs[0])), dev(torch.zeros(O, K)), dev(torch.zeros(O, K))]
            out = k.linear_bwd_weight_group([dev(t) for t in dys_], [dev(t) for t in xs_], dws, [False, True, True])
            assert all(a is b for a, b in zip(out, dws))
            for dw, dy, x in zip(dws, dys_, xs_):
                close(dw, dy.double().T @ x.double(), rtol=TOL[mode])


@pytest.mark.parametrize("mode", ["fp32", "split"])
def test_gemm_grouped(cuda, mode):
    guarded(cuda, grouped_body, mode)


def colsum_body(rows, cols):
    from boosted_detr_amd import _lib, kernels as k
    x = rnd(rows, cols, seed=rows * 100 + cols)
    ref = x.double().sum(0)
    close(k.colsum(dev(x)), ref)                                            # the two-launch form: partial rows, then the fixed-order fold
    for det in (False, True):                                               # one launch of float atomics / the two-level form again
        prev = k.set_deterministic(det)
        try:
            acc = dev(torch.zeros(cols))
            k.colsum(dev(x), out=acc, prezeroed=True)
            close(acc, ref, rtol=1e-5)
        finally:
            k.set_deterministic(prev)
    if cols % 4:                                                            # "bdetr_colstats: bad arguments (C % 4 == 0 required)": refused, not run
        with pytest.raises(_lib.BdetrError, match="C % 4 == 0 required"):
            k.colstats(dev(x))
        return
    psum, psq, n = k.colstats(dev(x))
    assert tuple(psum.shape) == (n, cols)
    close(psum.sum(0), ref, rtol=1e-5)
    close(psq.sum(0), (x.double() ** 2).sum(0), rtol=1e-5)


@pytest.mark.parametrize("cols", [3, 64, 65])
@pytest.mark.parametrize("rows", [1, 31, 33])
def test_colsum_colstats(cuda, rows, cols):
    guarded(cuda, colsum_body, rows, cols)


def colsum_group_body(cols):
    from boosted_detr_amd import kernels as k
    rows = (1, 31, 33, 31)
    xs = [rnd(r, cols, seed=10 + i) for i, r in enumerate(rows)]
    base = [rnd(cols, seed=50 + i) for i in range(len(rows))]
    outs = [dev(b) for b in base]
    k.colsum_group([dev(x) for x in xs], outs)
    for x, b, o in zip(xs, base, outs):
        close(o, b.double() + x.double().sum(0), rtol=1e-5)
    arena().results.extend(("colsum_group", o) for o in outs)               # (the entry point returns nothing: its destinations are the results)


@pytest.mark.parametrize("cols", [3, 64, 65])
def test_colsum_group(cuda, cols):
    guarded(cuda, colsum_group_body, cols)


# ------------------------------------------------------------------------------------------------------------ fp32 convolution
def conv_case(N, H, W, C, K, R, stride, pad):
    """test_precision_gpu.conv_case under 'fp32' (same references and bars), except that a backward-data the entry point refuses -
    stride > 1 with overlapping taps: "stride>1 only for 1x1 convs or taps that do not overlap" - is asserted to BE refused instead
    of being skipped by name (that body skips R = 7 only)."""
    from boosted_detr_amd import _lib, kernels as k
    tol = TOL["fp32"]
    x, w, b = rnd(N, H, W, C, seed=1), rnd(K, R, R, C, seed=2, scale=(R * R * C) ** -0.5), rnd(K, seed=3)
    g = k.ConvGeom(N, H, W, C, K, R, R, stride, pad)
    y, (ps, pq, n) = k.conv2d_fwd(dev(x), dev(w), dev(b), g, 0, want_stats=True)
    xt = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    wt = w.double().permute(0, 3, 1, 2).requires_grad_(True)
    ref = F.conv2d(xt, wt, b.double(), stride=stride, padding=pad)
    r2 = ref.permute(0, 2, 3, 1).reshape(-1, K)
    close(y, ref.permute(0, 2, 3, 1), rtol=TOL_FWD["fp32"])
    close(ps.sum(0), r2.sum(0), rtol=1e-4)
    close(pq.sum(0), (r2 * r2).sum(0), rtol=1e-4)
    dy = rnd(*ref.shape, seed=4).double()
    ref.backward(dy)
    dyn = dy.permute(0, 2, 3, 1).float()
    if stride == 1 or R == 1 or (R <= stride and pad == 0):
        close(k.conv2d_bwd_data(dev(dyn), dev(w), g), xt.grad.permute(0, 2, 3, 1), rtol=tol)
        base = rnd(N, H, W, C, seed=9)
        dx2 = dev(base)
        k.conv2d_bwd_data(dev(dyn), dev(w), g, dx=dx2, accumulate=True)
        close(dx2, base.double() + xt.grad.permute(0, 2, 3, 1), rtol=tol)
    else:
        with pytest.raises(_lib.BdetrError, match="stride>1 only for 1x1"):
            k.conv2d_bwd_data(dev(dyn), dev(w), g)
    close(k.conv2d_bwd_weight(dev(x), dev(dyn), g), wt.grad.permute(0, 2, 3, 1), rtol=max(tol, 5e-5))


def conv_body(N, H, W, C, K, R, stride, pad):
    from boosted_detr_amd import kernels as k
    with k.gemm_precision("fp32"):
        for det in (False, True):                       # deterministic: split-K through guarded slabs + a fixed-order fold
            prev = k.set_deterministic(det)
            try:
                conv_case(N, H, W, C, K, R, stride, pad)
            finally:
                k.set_deterministic(prev)


@pytest.mark.parametrize("N,H,W,C,K,R,stride,pad", [(1, 1, 1, 4, 4, 1, 1, 0), (1, 9, 11, 128, 32, 3, 1, 1), (2, 5, 7, 8, 12, 3, 2, 1), (1, 13, 17, 4, 64, 7, 2, 3)])
def test_conv_fp32(cuda, N, H, W, C, K, R, stride, pad):
    guarded(cuda, conv_body, N, H, W, C, K, R, stride, pad)


def conv_stride4_body(N, H, C, Kc):
    """test_panoptic_train_gpu.test_conv_out_3x3_stride4_backward with the running sum placed by `dev` (not cloned outside the arena)."""
    from boosted_detr_amd import kernels as k
    g = k.ConvGeom(N, H, H, C, Kc, 3, 3, 4, 0)
    x, w, dy = rnd(N, H, H, C, seed=1), rnd(Kc, 3, 3, C, seed=2, scale=0.1), rnd(N, g.OH, g.OW, Kc, seed=3)
    xd, wd = x.double().permute(0, 3, 1, 2).requires_grad_(), w.double().permute(0, 3, 1, 2).requires_grad_()
    F.conv2d(xd, wd, stride=4).backward(dy.double().permute(0, 3, 1, 2))
    base = rnd(N, H, H, C, seed=4)
    with k.gemm_precision("fp32"):
        dx = k.conv2d_bwd_data(dev(dy), dev(w), g)
        dw = k.conv2d_bwd_weight(dev(x), dev(dy), g)
        acc = dev(base)
        k.conv2d_bwd_data(dev(dy), dev(w), g, dx=acc, accumulate=True)
    close(dx, xd.grad.permute(0, 2, 3, 1), rtol=2e-5)
    close(dw, wd.grad.permute(0, 2, 3, 1), rtol=5e-5)
    close(acc, base.double() + xd.grad.permute(0, 2, 3, 1), rtol=2e-5)
    assert float(dx[:, 11:].abs().max()) == 0.0 and float(dx[:, 3::4].abs().max()) == 0.0      # rows no window reaches: written, as zeros


def test_conv_3x3_stride4(cuda):
    guarded(cuda, conv_stride4_body, 2, 13, 8, 12)


# ------------------------------------------------------------------------------------------------------------ P16 path
def p16_pack_body(n):
    from boosted_detr_amd import kernels as k
    x = rnd(n, seed=n) * 3
    x[:8] = torch.tensor([0.0, -0.0, 1e-8, -3e-5, 65000.0, 1e-3, 255.5, -1.0])
    f, b = k.p16_pack(dev(x))
    assert torch.equal(test_p16_gpu.bits(f), test_p16_gpu.p16_ref(x, True)) and torch.equal(test_p16_gpu.bits(b), test_p16_gpu.p16_ref(x, False))
    xf, xb = k.p16_unpack(f, True).cpu(), k.p16_unpack(b, False).cpu()
    assert bool(((xf - x).abs() <= x.abs() * 2.0 ** -21 + 2.0 ** -25).all()) and bool(((xb - x).abs() <= x.abs() * 2.0 ** -15 + 1e-30).all())
    only_f, none_b = k.p16_pack(dev(x), want_bf16=False)
    assert none_b is None and torch.equal(only_f, f)
    assert int(k.overflow_flag().item()) == 0


@pytest.mark.parametrize("n", [8, 24, 264])
def test_p16_pack_unpack(cuda, n):
    guarded(cuda, p16_pack_body, n)


def test_p16_weight_packs(cuda):
    guarded(cuda, test_p16_gpu.test_weight_packs_bit_exact, cuda)


@pytest.mark.parametrize("rows,C", [(51, 8), (98, 2048)])
def test_bn_p16(cuda, rows, C):
    """bn_apply_p16 / bn_bwd_p16 with a residual, the f16-pair residual, the bf16-pair and the bit-mask ReLU sources (want_mask)."""
    guarded(cuda, test_p16_gpu.test_bn_p16_producers_match_the_fp32_kernels, cuda, rows, C, True, True)


def test_relu_mask_apply_and_masked_accumulate(cuda):
    guarded(cuda, test_p16_gpu.test_masked_skip_accumulate_in_the_bwd_data_epilogue, cuda, 1, 5, 6, 40, 72)


def even_apply_body(N, H, W, C):
    """bn_apply_p16(even_pixels): the pixels (2i, 2j) equal the dense launch's, every other pixel - a second kind of "outside" - keeps
    the arena's fill byte in all four outputs (tests/test_even_apply_gpu.py checks the same through buffers of its own)."""
    from boosted_detr_amd import kernels as k
    a = arena()
    rows = N * H * W
    y = dev(rnd(rows, C, seed=3) * 2 + 0.3)
    gamma, beta = dev(1 + 0.1 * rnd(C, seed=4)), dev(0.1 * rnd(C, seed=5))
    mean, rstd = k.bn_stats(rows, C, k.colstats(y), 1.001e-5, 0.99, True, dev(torch.zeros(C)), dev(torch.ones(C)), like=y)
    res = dev(rnd(rows, C, seed=6))
    dense = k.bn_apply_p16(y, mean, rstd, gamma, beta, res, True, want_mask=True)
    even = k.bn_apply_p16(y, mean, rstd, gamma, beta, res, True, want_mask=True, even_pixels=(H, W))
    a.mark_partial(*even)                                                    # by contract partly unwritten; checked right here instead
    on = torch.zeros(N, H, W, dtype=torch.bool)
    on[:, ::2, ::2] = True
    fill = a.fill
    for name, d, e in zip(("out32", "f16 pair", "bf16 pair", "mask"), dense, even):
        d8, e8 = d.cpu().view(torch.uint8).view(N, H, W, -1), e.cpu().view(torch.uint8).view(N, H, W, -1)
        assert torch.equal(e8[on], d8[on]), (name, "even pixels differ from the dense launch")
        assert bool((e8[~on] == fill).all()), (name, "an odd pixel was written")
        assert not bool((d8[~on] == fill).all())


@pytest.mark.parametrize("N,H,W,C", [(2, 2, 2, 256), (2, 4, 6, 512)])
def test_even_pixel_apply(cuda, N, H, W, C):
    guarded(cuda, even_apply_body, N, H, W, C)


# ------------------------------------------------------------------------------------------------------------ norms
def batchnorm_body(rows, C, relu, res):
    """test_kernels_gpu.test_batchnorm_train; a single row has no Bessel correction and no gradient through its own statistics."""
    if rows > 1:
        return test_kernels_gpu.test_batchnorm_train(None, rows, C, relu, res)
    from boosted_detr_amd import kernels as k
    x, gamma, beta = rnd(1, C, seed=1) * 2 + 0.5, 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
    mm, mv = rnd(C, seed=4), rnd(C, seed=5).abs() + 0.5
    resid = rnd(1, C, seed=6) if res else None
    mmd, mvd = dev(mm), dev(mv)
    mean, rstd = k.bn_stats(1, C, k.colstats(dev(x)), 1.001e-5, 0.99, False, mmd, mvd, like=mmd)
    out = k.bn_apply(dev(x), mean, rstd, dev(gamma), dev(beta), dev(resid) if res else None, relu)
    ref = beta.double().view(1, C) + (resid.double() if res else 0)          # (x - mean) = 0 exactly
    ref = ref.relu() if relu else ref
    close(out, ref)
    close(mean, x.double().view(C))
    # var = fl(x * x) - x * x: the rounding residue of the fp32 square, up to 2^-24 x^2 against eps = 1e-5 - rstd is bounded, not pinned
    assert bool((rstd > 0).all()) and float(rstd.max()) <= 316.1
    close(mmd, mm.double() * 0.99 + x.double().view(C) * 0.01)
    close(mvd, mv.double() * 0.99)
    dout = rnd(1, C, seed=7)
    dx, dg, db, dres = k.bn_bwd(dev(dout), out, dev(x), mean, rstd, dev(gamma), relu, False, want_residual_grad=res)
    g = dout.double() * ((ref > 0) if relu else 1)
    close(db, g.view(C))
    assert float(dg.abs().max()) <= 1e-4 * float(g.abs().max()) and float(dx.abs().max()) <= 1e-4 * float(g.abs().max()) * 316.1    # xhat = 0; rstd = eps^-1/2 = 316.1
    if res:
        close(dres, g)


@pytest.mark.parametrize("C", [4, 8, 64, 2048])
@pytest.mark.parametrize("rows", [1, 31, 33, 98])
def test_batchnorm(cuda, rows, C):
    guarded(cuda, batchnorm_body, rows, C, True, True)
    guarded(cuda, batchnorm_body, rows, C, False, False)


def frozen_body(rows, C):
    from boosted_detr_amd import kernels as k
    x, gamma, beta = rnd(rows, C, seed=1), 1 + 0.1 * rnd(C, seed=2), rnd(C, seed=3)
    mm, mv = rnd(C, seed=4), rnd(C, seed=5).abs() + 0.5
    mean, rstd = k.bn_stats_frozen(dev(mm), dev(mv), 1e-3)
    close(mean, mm.double()); close(rstd, (mv.double() + 1e-3) ** -0.5)
    out = k.bn_apply(dev(x), mean, rstd, dev(gamma), dev(beta), None, False)
    xd = x.double().requires_grad_(True)
    ref = (xd - mm.double()) / torch.sqrt(mv.double() + 1e-3) * gamma.double() + beta.double()
    close(out, ref)
    dout = rnd(rows, C, seed=7)
    ref.backward(dout.double())
    dx, dg, db, _ = k.bn_bwd(dev(dout), out, dev(x), mean, rstd, dev(gamma), False, True)
    close(dx, xd.grad)


@pytest.mark.parametrize("rows,C", [(1, 4), (33, 8), (98, 2048)])
def test_batchnorm_frozen(cuda, rows, C):
    guarded(cuda, frozen_body, rows, C)


@pytest.mark.parametrize("G,R,C", [(4, 7, 64), (2, 65, 48)])
def test_grouped_rows_batchnorm(cuda, G, R, C):
    guarded(cuda, test_aux_losses_gpu.test_grouped_batchnorm_training, cuda, G, R, C)
    guarded(cuda, test_aux_losses_gpu.test_grouped_batchnorm_frozen, cuda, G, R, C)


def layernorm_body(rows, D, rate):
    """test_kernels_gpu.test_add_dropout_layernorm without its check of the kept fraction (a statement about 20,000 draws, not about
    64): the keep mask is recovered from a probe run in the same way, references and tolerances are that test's."""
    from boosted_detr_amd import kernels as k
    x, y = rnd(rows, D, seed=1), rnd(rows, D, seed=2)
    gamma, beta = 1 + 0.1 * rnd(D, seed=3), 0.1 * rnd(D, seed=4)
    out, mean, rstd = k.add_dropout_layernorm_fwd(dev(x), dev(y), dev(gamma), dev(beta), 1e-3, rate, 1234)
    keep = torch.ones(rows, D, dtype=torch.float64)
    if rate:
        o2, m2, r2 = k.add_dropout_layernorm_fwd(dev(torch.zeros(rows, D)), dev(torch.ones(rows, D)), dev(torch.ones(D)), dev(torch.zeros(D)), 1e-3, rate, 1234)
        h = o2.cpu().double() / r2.cpu().double()[:, None] + m2.cpu().double()[:, None]
        keep = (h > 0.5).double() / (1 - rate)
    xd, yd = x.double().requires_grad_(True), y.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ref = F.layer_norm(xd + yd * keep, (D,), gd, bd, 1e-3)
    close(out, ref)
    dout = rnd(rows, D, seed=5)
    ref.backward(dout.double())
    dx, dy, dg, db = k.add_dropout_layernorm_bwd(dev(dout), dev(x), dev(y), dev(gamma), mean, rstd, rate, 1234)
    close(dx, xd.grad, rtol=1e-4); close(dy, yd.grad, rtol=1e-4); close(dg, gd.grad, rtol=1e-4); close(db, bd.grad, rtol=1e-4)


@pytest.mark.parametrize("rate", [0.0, 0.1])
@pytest.mark.parametrize("rows,D", [(1, 64), (37, 64), (5, 1024)])
def test_add_dropout_layernorm(cuda, rows, D, rate):
    guarded(cuda, layernorm_body, rows, D, rate)


@pytest.mark.parametrize("rows,cols", [(1, 1), (7, 3), (5, 1050)])
def test_softmax_rows(cuda, rows, cols):
    guarded(cuda, test_kernels_gpu.test_softmax, cuda, rows, cols)


# ------------------------------------------------------------------------------------------------------------ attention, row chain
def attention_one_key_body(B, h, nq, policy):
    """nk = 1: the softmax is 1, o = v, dv = sum over the queries of dO, and dq = dk = 0 exactly in the reference - a bar relative to
    max|ref| means nothing there.  dS = P (dP - D) carries the product error of dP and D relative to |dP| (test_fused_attention_fwd_bwd's
    own remark), and dq = scale dS k: |dq - 0| <= tol * max_q sum_d |dO||v| * max|k| * scale; dk likewise with max|q| and nq terms."""
    from boosted_detr_amd import kernels as k
    D = h * 32
    Q, Kt, V, dO = rnd(B, nq, D, seed=1), rnd(B, 1, D, seed=2), rnd(B, 1, D, seed=3), rnd(B, h, nq, 32, seed=4)
    scale = 1.0 / np.sqrt(32.0)
    with k.gemm_precision(policy):
        o, lse = k.attention_fwd(dev(Q), dev(Kt), dev(V), h, scale)
        dq, dk, dv = k.attention_bwd(dev(Q), dev(Kt), dev(V), o, dev(dO), lse, h, scale)
    fwd_tol = 5e-5 if policy == "bf16x3" else 1e-5
    bwd_tol = 5e-5 if policy == "fp32" else 2e-4
    Vh = V.double().view(B, 1, h, 32).permute(0, 2, 1, 3)
    close(o, Vh.expand(B, h, nq, 32), rtol=fwd_tol)
    s = (Q.double().view(B, nq, h, 32).permute(0, 2, 1, 3) * Kt.double().view(B, 1, h, 32).permute(0, 2, 1, 3)).sum(-1) * scale
    close(lse, s, rtol=fwd_tol)
    close(dv, dO.double().sum(2).reshape(B, 1, D), rtol=bwd_tol)
    dp = float((dO.double().abs() * Vh.abs()).sum(-1).max())
    assert float(dq.abs().max()) <= bwd_tol * dp * float(Kt.abs().max()) * scale
    assert float(dk.abs().max()) <= bwd_tol * dp * float(Q.abs().max()) * scale * nq


# nq = 1 and nk = 1: bdetr_attention_* admits every nq, nk > 0 (csrc/attention.hip check_common)
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("B,h,nq,nk", [(1, 4, 50, 49), (2, 8, 49, 49), (1, 8, 33, 65), (1, 4, 1, 49), (1, 4, 50, 1), (1, 4, 1, 1)])
def test_attention(cuda, B, h, nq, nk, policy):
    if nk == 1:
        guarded(cuda, attention_one_key_body, B, h, nq, policy)
    else:
        guarded(cuda, test_kernels_gpu.test_fused_attention_fwd_bwd, cuda, B, h, nq, nk, policy)


def rowchain_body(M, nstages):
    """test_rowchain_gpu.test_rowchain_kernels_match_fp64 with the packed weight copies and the reduce destinations in the arena."""
    from boosted_detr_amd import _lib, kernels as k
    D = test_rowchain_gpu.D
    a = arena()
    p = test_rowchain_gpu.make_params(10)
    ctx, resid, dout = rnd(M, D, seed=1), rnd(M, D, seed=2), rnd(M, D, seed=3)
    n = int(_lib.lib().bdetr_rowchain_pack_elems())
    names = ["Wo", "W1", "W2"][:nstages]
    wdev = {w: dev(p[w]) for w in names}
    like = wdev["Wo"]
    fwd, bwd = {w: k.empty(n, like=like) for w in names}, {w: k.empty(n, like=like) for w in names}
    table = dev(torch.tensor([[wdev[w].data_ptr(), fwd[w].data_ptr(), bwd[w].data_ptr()] for w in names], dtype=torch.int64), torch.int64)
    k.rowchain_pack_weights(table)
    a.results.extend(("rowchain_pack_weights", t) for t in list(fwd.values()) + list(bwd.values()))
    biases = [dev(p[b]) for b in ["bo", "b1", "b2"][:nstages]]
    ln1, ln2 = (dev(p["g1"]), dev(p["be1"])), ((dev(p["g2"]), dev(p["be2"])) if nstages == 3 else None)
    saved = k.rowchain_fwd(dev(ctx), dev(resid), [fwd[w] for w in names], biases, ln1, ln2, 1e-3, 0.0, 0, 0, None)
    pd = {kk: v.double().requires_grad_(True) for kk, v in p.items()}
    cd, rd = ctx.double().requires_grad_(True), resid.double().requires_grad_(True)
    ref = test_rowchain_gpu.chain_ref(cd, rd, pd, nstages)
    for key in ("pre1", "x1") + (("h", "pre2", "x2") if nstages == 3 else ()):
        close(saved[key], ref[key], rtol=3e-5)
    close(saved["mean1"], ref["pre1"].mean(-1), rtol=3e-5, atol=3e-5 * float(ref["pre1"].detach().abs().max()))
    close(saved["rstd1"], 1.0 / torch.sqrt(ref["pre1"].var(-1, unbiased=False) + 1e-3), rtol=3e-5)
    ref["out"].backward(dout.double())
    gammas = (ln1[0],) + ((ln2[0],) if nstages == 3 else ())
    dctx, dres, G, partials, nparts = k.rowchain_bwd(dev(dout), saved, [bwd[w] for w in names], gammas, 0.0, 0, 0, None)
    close(dctx, cd.grad, rtol=2e-4); close(dres, rd.grad, rtol=2e-4)
    if nstages == 1:
        # one stage writes the vectors 4..6 of every partial row only (kernels.rowchain_reduce: "dsts: 7 tensors or None"): the other four
        # keep the fill - checked here, bit for bit - and the partial rows are exempt from the NaN check
        a.mark_partial(partials)
        host = partials.cpu()
        assert not bool(torch.isnan(host[:, 4:]).any())
        assert bool((host[:, :4].contiguous().view(torch.uint8) == a.fill).all())
    vec = [dev(torch.full((D,), float("nan"))) for _ in range(7)]            # accumulate = 0: the old content must not matter
    dsts = vec if nstages == 3 else [None] * 4 + vec[4:]
    k.rowchain_reduce(partials, nparts, dsts, [0] * 7)
    a.results.extend(("rowchain_reduce", t) for t in dsts if t is not None)
    want = [pd["g2"].grad, pd["be2"].grad, pd["b2"].grad, pd["b1"].grad, pd["g1"].grad, pd["be1"].grad, pd["bo"].grad]
    for i in range(7):
        if nstages == 3 or i >= 4:
            close(vec[i], want[i], rtol=2e-4)
    base = rnd(D, seed=77)
    acc = dev(base)                                                         # accumulate = 1 onto a running sum
    k.rowchain_reduce(partials, nparts, [None] * 6 + [acc], [0] * 6 + [1])
    close(acc, base.double() + want[6], rtol=2e-4)
    xs = [ctx] + ([ref["x1"].detach(), ref["h"].detach()] if nstages == 3 else [])
    for g, x, w in zip(G, xs, names):
        close(g.double().cpu().T @ x.double(), pd[w].grad, rtol=2e-4)


@pytest.mark.parametrize("nstages", [1, 3])
@pytest.mark.parametrize("M", [1, 33, 98])
def test_rowchain(cuda, M, nstages):
    guarded(cuda, rowchain_body, M, nstages)


# ------------------------------------------------------------------------------------------------------------ stem, input step
@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (1, 2, 3), (3, 13, 17)])
def test_stem_pool(cuda, N, H, W):
    guarded(cuda, test_stem_gpu.test_stem_pool_matches_the_unfused_kernels_and_fp64, cuda, N, H, W)


def stem_wgrad_body(N, H, W):
    """test_stem_gpu.test_stem_weight_gradient_on_the_space_to_depth_path with a guarded destination (prefilled with NaN: every
    element is overwritten)."""
    from boosted_detr_amd import kernels as k
    K_ = 64
    x = rnd(N, H, W, 4, seed=1, scale=40.0)
    x[..., 3] = 0
    dy = rnd(N, H // 2, W // 2, K_, seed=2)
    wt = torch.zeros(K_, 4, 7, 7, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().permute(0, 3, 1, 2), wt, stride=2, padding=3).backward(dy.double().permute(0, 3, 1, 2))
    want = wt.grad.permute(0, 2, 3, 1).contiguous()
    with k.gemm_precision("split"):
        _, dyb = k.p16_pack(dev(dy), want_f16=False)
        got = k.stem_bwd_weight_s2d(dev(x), dyb, dev(torch.full((K_, 7, 7, 4), float("nan"))))
    scale = float(want.abs().max())
    assert float((got.double().cpu() - want).abs().max()) <= 3e-5 * scale


def test_stem_weight_gradient_s2d(cuda):
    guarded(cuda, stem_wgrad_body, 3, 18, 22)


def maxpool_body(N, H, W, C):
    from boosted_detr_amd import kernels as k
    x = rnd(N, H, W, C, seed=1).relu()
    y = k.maxpool_fwd(dev(x))
    xt = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    ref = F.max_pool2d(F.pad(xt, (1, 1, 1, 1)), 3, 2)
    close(y, ref.permute(0, 2, 3, 1), rtol=0, atol=0)
    dy = rnd(*ref.shape, seed=2).double()
    ref.backward(dy)
    dx = k.maxpool_bwd(dev(x), y, dev(dy.permute(0, 2, 3, 1).float()))
    m = (x > 0).double()                                                    # ties at zero are masked by the producer's ReLU
    close(dx.cpu().double() * m, xt.grad.permute(0, 2, 3, 1) * m)


@pytest.mark.parametrize("N,H,W,C", [(1, 1, 1, 4), (2, 15, 18, 64)])
def test_maxpool(cuda, N, H, W, C):
    guarded(cuda, maxpool_body, N, H, W, C)


def image_prep_body(H, W):
    from boosted_detr_amd import kernels as k
    from oracle import detr_oracle as O
    img = (np.random.default_rng(0).random((2, 5, 7, 3), dtype=np.float32) * 1.2 - 0.1).astype(np.float32)
    ref = O.Net(O.Config(image_size=(H, W)), {}, torch.float32).image_prep(torch.from_numpy(img))
    out = k.image_prep(dev(img), H, W).cpu()
    assert (out[..., 3] == 0).all()
    if (H, W) == (5, 7):
        assert torch.equal(out[..., :3], ref)                               # integer pixel values: bit-exact
    else:
        # test_kernels_gpu.test_image_prep: the uint8 truncation may flip by one unit where the interpolant lands within round-off of
        # an integer, for fewer than 1 element in 1000 - at 384 elements: rounded up to one element
        diff = (out[..., :3] - ref).abs()
        assert diff.max() <= 1.0 and int((diff > 0).sum()) <= 1, (float(diff.max()), int((diff > 0).sum()))


@pytest.mark.parametrize("H,W", [(5, 7), (8, 8)])
def test_image_prep(cuda, H, W):
    guarded(cuda, image_prep_body, H, W)


def _augment_params(B, H, W):
    from boosted_detr_amd.pipeline import Augmentations
    p = Augmentations(seed=5, jpeg_quality=False).draw(B, H, W)
    p["rand_val"][0] = [1.0, 1.0]; p["new_h"][0], p["new_w"][0], p["off_h"][0], p["off_w"][0] = H, W, 0, 0               # identity geometry
    p["rand_val"][1] = [1.7, 1.3]; p["new_h"][1], p["new_w"][1] = int(np.float32(H) / np.float32(1.7)), int(np.float32(W) / np.float32(1.3))
    p["off_h"][1], p["off_w"][1] = H - p["new_h"][1], W - p["new_w"][1]                                                   # flush with the bottom right corner
    return p


def augment_body(H, W):
    """tests/test_pipeline.py::test_gpu_augment_matches_oracle through kernels.augment itself: fp32 against the fp64 oracle to 2e-5
    without the JPEG round trip; with it the comparison is that test's statistical one (the codec is compared bit for bit below)."""
    from boosted_detr_amd import kernels as k
    from oracle import augment_oracle as AO
    B = 2
    image = np.random.default_rng(1).random((B, H, W, 3), dtype=np.float32)
    p = _augment_params(B, H, W)
    quality = p.pop("jpeg_quality")
    ip = np.stack([p["new_h"], p["new_w"], p["off_h"], p["off_w"]], axis=-1).astype(np.int32)
    fp = np.stack([p["contrast"], p["brightness"], p["saturation"]], axis=-1).astype(np.float32)
    got = k.augment(dev(image), dev(ip, torch.int32), dev(fp)).cpu().numpy().astype(np.float64)
    for b in range(B):
        err = np.abs(got[b] - AO.augment(image[b], p, b)).max()
        assert err < 2e-5, (b, err)
    p["jpeg_quality"] = quality
    got = k.augment(dev(image), dev(ip, torch.int32), dev(fp), dev(quality, torch.int32)).cpu().numpy().astype(np.float64)
    for b in range(B):
        d = np.abs(got[b] - AO.augment(image[b], p, b))
        assert d.mean() < 0.5 / 255, (b, d.mean(), d.max())
        if d.size >= 768:                                                   # "99 % of the values": a statement about at least a few hundred of them
            assert (d <= 4.0 / 255).mean() > 0.99, (b, d.mean(), d.max())


def jpeg_body(H, W):
    """tests/test_jpeg_quality.py::test_gpu_jpeg_quality_is_bit_exact_against_the_oracle at B = 2; the JPEG workspace is a guarded
    scratch buffer (margins only)."""
    from boosted_detr_amd import kernels as k
    from oracle import jpeg_oracle as J
    rng = np.random.default_rng(H * 1000 + W)
    u8 = rng.integers(0, 256, (2, H, W, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    u8[1] = np.clip(np.stack([128 + 100 * np.sin(xx / 7.0 + yy / 11.0), 128 + 90 * np.cos(xx / 5.0), 128 + 80 * np.sin(yy / 3.0)], -1)
                    + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
    image = ((u8.astype(np.float64) + 0.5) / 255.5).astype(np.float32)
    quality = np.array([70, 99], np.int32)
    got = k.jpeg_quality(dev(image), dev(quality, torch.int32)).cpu().numpy()
    for b in range(2):
        want = J.jpeg_quality_roundtrip_u8(u8[b], int(quality[b]))
        assert np.array_equal(np.rint(got[b].astype(np.float64) * 255.0).astype(np.int64), want.astype(np.int64))
        assert np.array_equal(got[b], want.astype(np.float32) / np.float32(255.0))


# 17 x 33: one row and one column past a 16 x 16 MCU
@pytest.mark.parametrize("H,W", [(5, 7), (16, 16), (17, 33)])
def test_augment_and_jpeg_quality(cuda, H, W):
    guarded(cuda, augment_body, H, W)
    guarded(cuda, jpeg_body, H, W)


# ------------------------------------------------------------------------------------------------------------ panoptic head
def panoptic_forward_body():
    """test_panoptic_gpu.test_panoptic_pieces with a guarded copy_cols destination and the small resize targets."""
    from boosted_detr_amd import kernels as k
    x = rnd(2, 7, 9, 8, seed=1)
    for (H, W) in ((5, 4), (7, 9)):
        ref = F.interpolate(x.double().permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        close(k.resize_bilinear(dev(x), H, W), ref, rtol=1e-5)
    for C in (5, 29, 254):
        ld = k.pad4(C) + 4                                                  # padding columns hold garbage the kernel must ignore
        t = rnd(3, 5, 5, ld, seed=2)
        g, b = 1 + 0.1 * rnd(C, seed=3), 0.1 * rnd(C, seed=4)
        ref = F.leaky_relu(F.layer_norm(t[..., :C].double(), (C,), g.double(), b.double(), 1e-3), 0.01)
        out = k.layernorm_act(dev(t), C, dev(g), dev(b), 1e-3, 0.01)
        assert out.shape[-1] == k.pad4(C) and (k.pad4(C) == C or float(out[..., C:].abs().max()) == 0.0)
        close(out[..., :C], ref, rtol=1e-5)
        base = rnd(3, 5, 5, C + 15, seed=5)
        dst = dev(base)
        k.copy_cols(out, C, dst, 10)
        assert torch.equal(dst[..., 10:10 + C], out[..., :C])
        assert torch.equal(dst[..., :10].cpu(), base[..., :10]) and torch.equal(dst[..., 10 + C:].cpu(), base[..., 10 + C:])      # columns outside the slice: untouched
        assert torch.equal(k.nhwc_to_nchw(out, C), out[..., :C].permute(0, 3, 1, 2).reshape(3, C, 25))


def test_panoptic_forward_pieces(cuda):
    guarded(cuda, panoptic_forward_body)


@pytest.mark.parametrize("C", [5, 29, 254])
def test_panoptic_layernorm_act_bwd(cuda, C):
    guarded(cuda, test_panoptic_train_gpu.test_layernorm_act_bwd, cuda, C, 0.01)


@pytest.mark.parametrize("src,dst", [((7, 9), (5, 4)), ((7, 9), (7, 9))])
def test_panoptic_resize_bwd(cuda, src, dst):
    guarded(cuda, test_panoptic_train_gpu.test_resize_bilinear_bwd, cuda, src, dst)


def weight_pack_body(shape, transpose):
    """test_panoptic_train_gpu.test_weight_pack_and_unpack with guarded unpack destinations (prefilled with NaN)."""
    from boosted_detr_amd import kernels as k
    kern = rnd(*shape, seed=1).numpy()
    Kc = shape[2] if transpose else shape[3]
    bias = rnd(Kc, seed=2).numpy()
    w, b = k.conv_weight_pack(dev(kern), dev(bias), transpose)
    want_w, want_b = test_panoptic_train_gpu._numpy_pack(kern, bias, transpose)
    assert np.array_equal(w.cpu().numpy(), want_w) and np.array_equal(b.cpu().numpy(), want_b)
    dw, db = rnd(*want_w.shape, seed=3), rnd(*want_b.shape, seed=4)
    dk, dbias = dev(torch.full(shape, float("nan"))), dev(torch.full((Kc,), float("nan")))
    k.conv_weight_unpack(dev(dw), dev(db), shape, transpose, dk, dbias)
    kt, bt = torch.from_numpy(kern).double().requires_grad_(), torch.from_numpy(bias).double().requires_grad_()
    packed = kt.flip(0, 1).permute(2, 0, 1, 3) if transpose else kt.permute(3, 0, 1, 2)
    ((packed * dw[:Kc, :, :, :packed.shape[3]].double()).sum() + (bt * db[:Kc].double()).sum()).backward()
    assert torch.equal(dk.cpu().double(), kt.grad) and torch.equal(dbias.cpu().double(), bt.grad)


@pytest.mark.parametrize("shape,transpose", [((2, 2, 29, 19), False), ((2, 2, 43, 29), True)])
def test_panoptic_weight_pack(cuda, shape, transpose):
    guarded(cuda, weight_pack_body, shape, transpose)


def test_panoptic_layout_and_mask_loss(cuda):
    guarded(cuda, test_panoptic_train_gpu.test_nchw_to_nhwc_is_the_adjoint_of_nhwc_to_nchw, cuda)
    guarded(cuda, test_panoptic_train_gpu.test_mask_loss_kernel, cuda)


# ------------------------------------------------------------------------------------------------------------ set criterion
def criterion_body(B, M, N, C, A, nobj):
    """test_matcher_gpu.test_cost_lsa_loss_vs_oracle with every operand placed by `dev` and num_objects given (0 and M among them)."""
    from boosted_detr_amd import kernels as k
    from oracle import detr_oracle as O
    cfg = O.Config(num_object_preds=N, num_categories=C, num_attributes=A, attribute_weight=1.0)
    batch = O.make_batch(cfg, B, M, seed=5, image_hw=(8, 8), num_objects=list(nobj))
    rng = np.random.default_rng(1)
    cat = torch.softmax(torch.from_numpy(rng.standard_normal((B, N, C)).astype(np.float32) * 2), -1).numpy()
    att = torch.sigmoid(torch.from_numpy(rng.standard_normal((B, N, A)).astype(np.float32) * 3)).numpy()
    box = (rng.random((B, N, 4)) * np.array([0.7, 0.7, 0.5, 0.5])).astype(np.float32)
    box[:, ::7, 2] *= -1.0
    lo, g_cat, g_att, g_box = test_matcher_gpu._oracle_loss(cfg, batch, cat, att, box)
    att_hot = F.one_hot(torch.from_numpy(batch["attribute"].astype(np.int64)), A).amax(2).float()
    d = k.loss_desc(B, M, N, C, A, 1000.0, 1.0, 1.0, 100.0)
    args = (dev(cat), dev(att), dev(box), dev(batch["category"], torch.int32), dev(att_hot), dev(batch["bbox"]), dev(batch["num_objects"], torch.int32))
    cost, comps = k.cost_matrix(d, *args, components=True)
    n_obj = batch["num_objects"]
    assert 0 in n_obj.tolist() and M in n_obj.tolist()
    rowmask = (np.arange(M)[None, :] < n_obj[:, None])[:, :, None]
    ref_cost = lo.cost_total.detach().numpy() * rowmask
    assert np.abs(cost.cpu().numpy() - ref_cost).max() / np.abs(ref_cost).max() < 1e-5
    for got, want in zip(comps, lo.cost_components):
        w = want.detach().numpy() * rowmask
        assert np.abs(got.cpu().numpy() - w).max() <= 1e-5 * (np.abs(w).max() + 1e-12)
    match = k.lsa(cost, args[-1])
    assert np.array_equal(match.cpu().numpy(), test_matcher_gpu.scipy_match(cost.cpu().numpy(), n_obj))
    assert np.array_equal(k.match_to_mask(match, N).cpu().numpy(), lo.mask.numpy())
    losses, d_cat, d_att, d_box = k.set_loss(d, *args, match)
    want = torch.stack([lo.total, lo.category, lo.attribute, lo.box, lo.exist, lo.iou]).detach().numpy()
    assert np.abs(losses.cpu().numpy() - want).max() <= 2e-5 * np.abs(want).max()
    for gg, ww in ((d_cat, g_cat), (d_att, g_att), (d_box, g_box)):
        assert np.abs(gg.cpu().numpy() - ww.numpy()).max() <= 5e-5 * (np.abs(ww.numpy()).max() + 1e-12)


@pytest.mark.parametrize("B,M,N,C,A,nobj", [(3, 6, 8, 10, 6, (0, 6, 3)), (2, 12, 16, 48, 3, (12, 0))])
def test_set_criterion(cuda, B, M, N, C, A, nobj):
    guarded(cuda, criterion_body, B, M, N, C, A, nobj)


# ------------------------------------------------------------------------------------------------------------ optimizer
def test_adamw_flat_buffer(cuda):
    """The fused AdamW step (training.AdamW -> bdetr_adamw_clipnorm) over tensors of 1, 3, 257 and 1025 elements: each weight placed on
    its own between margins, the flat gradient / moment buffers and the norm scratch carved from the arena (the proxy stands in for
    `torch` in boosted_detr_amd.training too).  Two steps against tests/_adamw_ref.py at test_adamw_gpu's tolerance rule."""
    import _adamw_ref as R
    from boosted_detr_amd import kernels, training
    from boosted_detr_amd.engine import Variable
    from test_adamw_gpu import check_against_restatements, host
    sizes = [1, 3, 257, 1025]
    rng = np.random.default_rng(7)
    w = [(0.05 * rng.standard_normal(n)).astype(np.float32) for n in sizes]
    a = _guard.Arena(cuda)
    with a.armed((kernels, training)):
        vs = []
        for i, x in enumerate(w):
            v = Variable("syn/t%d/%s" % (i, "bias" if i == 1 else "kernel"), (x.size,))
            v.value = a.place(x, name="weight %d" % i)
            vs.append(v)
        opt = training.AdamW(1e-3, weight_decay=1e-2, clipnorm=R.CLIPNORM, exclude_from_weight_decay=R.EXCLUDE)
        opt.build(vs)
        m, v_ = [np.zeros_like(x) for x in w], [np.zeros_like(x) for x in w]
        for step in range(2):
            gs = [(rng.standard_normal(n) * (1e-3 if i == 0 else 1.0)).astype(np.float32) for i, n in enumerate(sizes)]
            for gv, g in zip(opt.grad_views, gs):
                gv.copy_(torch.from_numpy(g).to(gv.device))
            opt.apply_gradients()
            torch.cuda.synchronize()
            for i, var in enumerate(vs):
                kw = dict(lr=1e-3, wd=1e-2, t=step + 1, clipnorm=R.CLIPNORM, decay=i != 1)
                got = (host(var.value), host(opt.m_views[i]), host(opt.v_views[i]))
                for q, g_, r64, r32 in zip("wmv", got, R.adamw_step64(w[i], gs[i], m[i], v_[i], **kw), R.adamw_step32(w[i], gs[i], m[i], v_[i], **kw)):
                    check_against_restatements("%s[%d]" % (q, sizes[i]), g_, r64, r32, {})
                w[i], m[i], v_[i] = got
    weights = [v.value for v in vs]
    assert a.verify(weights + [opt.flat_grad, opt.flat_m, opt.flat_v, opt.d_norms], inplace=weights) == len(weights) + 4


# ------------------------------------------------------------------------------------------------------------ variable-length outputs
def rle_body():
    """mask_rle_encode on tests/_rle_ref.py's cases at one image size whose total count (827) is odd: `counts` is sized by a count
    pass, so its last element sits right in front of the margin."""
    import test_mask_rle_gpu as T
    from boosted_detr_amd import kernels as k
    masks, hw, clean, dirty, want = T.mixed_batch(((5, 65),))
    assert int(want[1][-1]) % 2 == 1
    for bits in (clean, dirty):
        counts, offset = k.mask_rle_encode(dev(bits.view(np.int64), None), dev(hw, None))
        torch.cuda.synchronize()
        T.assert_equal_to(want, counts, offset, "guarded")
    n_counts = k.mask_rle_count(dev(clean.view(np.int64), None), dev(hw, None))
    assert np.array_equal(n_counts.cpu().numpy().reshape(-1), np.diff(want[1]))


def test_mask_rle_encode(cuda):
    guarded(cuda, rle_body)


def test_mask_targets(cuda):
    """tests/_mask_raster_ref.py's cases at grid 4 with the bottom-edge placement (the host operands travel in one copy of their own;
    the masks and areas, sized from the pack, are carved from the arena)."""
    import test_mask_targets_gpu as T
    guarded(cuda, T.test_targets_bit_equal_to_reference, cuda, 4, T.PLACEMENTS[2])
