"""GPU parity tests of the individual HIP kernels (through the C ABI) against plain
PyTorch-CPU fp64 references of the same op.  Tolerances are stated per test (default:
max abs error <= 2e-5 x the reference's max magnitude, i.e. fp32 round-off over the sum)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def dev(a, dtype=torch.float32):
    t = torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a)
    return t.to(dtype).contiguous().cuda()


def close(got, want, rtol=2e-5, atol=None):
    got = got.detach().cpu().double()
    want = want.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = want.abs().max().item() + 1e-30
    err = (got - want).abs().max().item()
    tol = rtol * scale if atol is None else atol
    assert err <= tol, f"max err {err:.3e} > {tol:.3e} (scale {scale:.3e})"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# ---------------------------------------------------------------- GEMM
@pytest.mark.parametrize("M,K,O", [(300, 256, 256), (6400, 256, 256), (1600, 256, 1024), (100, 1024, 82), (130, 50, 48), (64, 32, 4)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear_fwd(cuda, M, K, O, act):
    from boosted_detr_amd import kernels as k
    x, w, b = rnd(M, K, seed=1), rnd(O, K, seed=2, scale=K ** -0.5), rnd(O, seed=3)
    y = k.linear_fwd(dev(x), dev(w), dev(b), act)
    ref = x.double() @ w.double().T + b.double()
    ref = [ref, ref.relu(), ref.tanh()][act]
    close(y, ref)


@pytest.mark.parametrize("M,K,O", [(300, 256, 256), (6400, 256, 1024), (100, 1024, 82), (130, 50, 48), (4000, 64, 64)])
def test_linear_bwd(cuda, M, K, O):
    from boosted_detr_amd import kernels as k
    x, w, dy = rnd(M, K, seed=1), rnd(O, K, seed=2), rnd(M, O, seed=3)
    dx = k.linear_bwd_data(dev(dy), dev(w))
    close(dx, dy.double() @ w.double())
    dw = k.linear_bwd_weight(dev(dy), dev(x))
    close(dw, dy.double().T @ x.double())
    db = k.colsum(dev(dy))
    close(db, dy.double().sum(0))
    acc = torch.zeros(O).cuda()
    k.colsum(dev(dy), out=acc, prezeroed=True)          # one-launch form: float atomics into a zero-filled gradient slot
    close(acc, dy.double().sum(0), rtol=1e-5)
    prev = k.set_deterministic(True)                    # bdetr_gemm_ws + the two-level column sum: bit-identical twice
    try:
        d1, d2 = k.linear_bwd_weight(dev(dy), dev(x)), k.linear_bwd_weight(dev(dy), dev(x))
        a1, a2 = torch.zeros(O).cuda(), torch.zeros(O).cuda()
        k.colsum(dev(dy), out=a1, prezeroed=True)
        k.colsum(dev(dy), out=a2, prezeroed=True)
    finally:
        k.set_deterministic(prev)
    close(d1, dy.double().T @ x.double())
    close(a1, dy.double().sum(0), rtol=1e-5)
    assert torch.equal(d1, d2) and torch.equal(a1, a2)


def test_colsum_group(cuda):
    """bdetr_colsum_accumulate_group: up to four column sums of one width in one launch (the Q / K / V bias gradients), ragged row counts,
    onto a running sum - against fp64."""
    from boosted_detr_amd import kernels as k
    for rows in ([6400, 6400, 6400], [1600, 6400, 6400, 33], [7, 1]):
        xs = [rnd(r, 256, seed=10 + i) for i, r in enumerate(rows)]
        base = [rnd(256, seed=50 + i) for i in range(len(rows))]
        outs = [dev(b) for b in base]
        k.colsum_group([dev(x) for x in xs], outs)
        for x, b, o in zip(xs, base, outs):
            close(o, b.double() + x.double().sum(0), rtol=1e-5)


def test_gemm_batched_attention_shapes(cuda):
    """QK^T, PV and dV with the [B,q,h,d] strides the attention block uses, incl. unaligned T=49."""
    from boosted_detr_amd import kernels as k
    for B, h, q, kk, d in [(2, 8, 100, 400, 32), (2, 8, 49, 49, 32), (3, 4, 50, 49, 16)]:
        D = h * d
        Q, Kt, V = rnd(B, q, D, seed=1), rnd(B, kk, D, seed=2), rnd(B, kk, D, seed=3)
        s = torch.empty(B, h, q, kk).cuda()
        k.gemm_raw(q, kk, d, dev(Q), D, True, dev(Kt), D, True, s, kk, nb0=B, nb1=h,
                   sa=(q * D, d), sb=(kk * D, d), sc=(h * q * kk, q * kk), alpha=0.25)
        Qh = Q.view(B, q, h, d).permute(0, 2, 1, 3).double()
        Kh = Kt.view(B, kk, h, d).permute(0, 2, 1, 3).double()
        Vh = V.view(B, kk, h, d).permute(0, 2, 1, 3).double()
        ref = 0.25 * Qh @ Kh.transpose(-1, -2)
        close(s, ref)
        p = torch.softmax(ref, -1).float()
        o = torch.empty(B, h, q, d).cuda()
        k.gemm_raw(q, d, kk, dev(p), kk, True, dev(V), D, False, o, d, nb0=B, nb1=h,
                   sa=(h * q * kk, q * kk), sb=(kk * D, d), sc=(h * q * d, q * d))
        close(o, p.double() @ Vh)
        dO = rnd(B, h, q, d, seed=4)
        dV = torch.empty(B, kk, D).cuda()
        k.gemm_raw(kk, d, q, dev(p), kk, False, dev(dO), d, False, dV, D, nb0=B, nb1=h,
                   sa=(h * q * kk, q * kk), sb=(h * q * d, q * d), sc=(kk * D, d))
        ref_dv = (p.double().transpose(-1, -2) @ dO.double()).permute(0, 2, 1, 3).reshape(B, kk, D)
        close(dV, ref_dv)


def test_gemm_accumulate_and_splitk(cuda):
    from boosted_detr_amd import kernels as k
    a, b = rnd(500, 320, seed=1), rnd(200, 320, seed=2)
    c0 = rnd(500, 200, seed=3)
    c = dev(c0)
    k.gemm_raw(500, 200, 320, dev(a), 320, True, dev(b), 320, True, c, 200, accumulate=True)
    close(c, c0.double() + a.double() @ b.double().T)
    c = torch.zeros(500, 200).cuda()
    k.gemm_raw(500, 200, 320, dev(a), 320, True, dev(b), 320, True, c, 200, splitk=3)
    close(c, a.double() @ b.double().T)


# ---------------------------------------------------------------- conv
CONVS = [  # N,H,W,C,K,R,stride,pad
    (2, 38, 38, 4, 64, 7, 2, 3),
    (2, 20, 20, 64, 64, 3, 1, 1),
    (2, 20, 20, 64, 256, 1, 1, 0),
    (2, 20, 20, 256, 128, 1, 2, 0),
    (1, 9, 11, 128, 32, 3, 1, 1),
    (3, 7, 7, 512, 2048, 1, 1, 0),
    (2, 14, 14, 256, 256, 3, 1, 1),
]


@pytest.mark.parametrize("N,H,W,C,K,R,stride,pad", CONVS)
def test_conv_fwd_bwd(cuda, N, H, W, C, K, R, stride, pad):
    from boosted_detr_amd import kernels as k
    x = rnd(N, H, W, C, seed=1)
    w = rnd(K, R, R, C, seed=2, scale=(R * R * C) ** -0.5)
    b = rnd(K, seed=3)
    g = k.ConvGeom(N, H, W, C, K, R, R, stride, pad)
    y, (ps, pq, n) = k.conv2d_fwd(dev(x), dev(w), dev(b), g, 0, want_stats=True)
    xt = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    wt = w.double().permute(0, 3, 1, 2).requires_grad_(True)
    ref = F.conv2d(xt, wt, b.double(), stride=stride, padding=pad)
    close(y, ref.permute(0, 2, 3, 1))
    r2 = ref.permute(0, 2, 3, 1).reshape(-1, K)
    close(ps.sum(0), r2.sum(0), rtol=1e-4)
    close(pq.sum(0), (r2 * r2).sum(0), rtol=1e-4)
    dy = rnd(*ref.shape, seed=4).double()
    ref.backward(dy)
    dyn = dy.permute(0, 2, 3, 1).float()
    if R != 7:
        dx = k.conv2d_bwd_data(dev(dyn), dev(w), g)
        close(dx, xt.grad.permute(0, 2, 3, 1))
        base = rnd(N, H, W, C, seed=9)
        dx2 = dev(base)
        k.conv2d_bwd_data(dev(dyn), dev(w), g, dx=dx2, accumulate=True)
        close(dx2, base.double() + xt.grad.permute(0, 2, 3, 1))
    dw = k.conv2d_bwd_weight(dev(x), dev(dyn), g)
    close(dw, wt.grad.permute(0, 2, 3, 1), rtol=5e-5)
    prev = k.set_deterministic(True)                    # split-K through slabs + a fixed-order fold (bdetr_conv2d_bwd_weight_ws)
    try:
        d1, d2 = k.conv2d_bwd_weight(dev(x), dev(dyn), g), k.conv2d_bwd_weight(dev(x), dev(dyn), g)
    finally:
        k.set_deterministic(prev)
    close(d1, wt.grad.permute(0, 2, 3, 1), rtol=5e-5)
    assert torch.equal(d1, d2)


# ---------------------------------------------------------------- norms
@pytest.mark.parametrize("rows,C,relu,res", [(800, 64, True, False), (3000, 256, True, True), (100, 1024, False, False), (98, 2048, False, False)])
def test_batchnorm_train(cuda, rows, C, relu, res):
    from boosted_detr_amd import kernels as k
    x = rnd(rows, C, seed=1) * 2 + 0.5
    gamma, beta = 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
    mm, mv = rnd(C, seed=4), rnd(C, seed=5).abs() + 0.5
    resid = rnd(rows, C, seed=6) if res else None
    eps = 1.001e-5
    mmd, mvd = dev(mm), dev(mv)
    parts = k.colstats(dev(x))
    mean, rstd = k.bn_stats(rows, C, parts, eps, 0.99, True, mmd, mvd, like=mmd)
    out = k.bn_apply(dev(x), mean, rstd, dev(gamma), dev(beta), dev(resid) if res else None, relu)
    xd = x.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rd = resid.double().requires_grad_(True) if res else None
    m, v = xd.mean(0), xd.var(0, unbiased=False)
    ref = (xd - m) / torch.sqrt(v + eps) * gd + bd
    if res:
        ref = ref + rd
    if relu:
        ref = ref.relu()
    close(out, ref)
    close(mean, m)
    close(mmd, mm.double() * 0.99 + m * 0.01)
    close(mvd, mv.double() * 0.99 + v * rows / (rows - 1) * 0.01)
    dout = rnd(rows, C, seed=7)
    ref.backward(dout.double())
    dx, dg, db, dres = k.bn_bwd(dev(dout), out, dev(x), mean, rstd, dev(gamma), relu, False, want_residual_grad=res)
    close(dx, xd.grad, rtol=1e-4)
    close(dg, gd.grad, rtol=1e-4)
    close(db, bd.grad, rtol=1e-4)
    if res:
        close(dres, rd.grad)
    elif relu:
        # mask recomputed from x (no read of `out`): identical result
        dx2, dg2, db2, _ = k.bn_bwd(dev(dout), None, dev(x), mean, rstd, dev(gamma), True, False, beta=dev(beta))
        assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db)


@pytest.mark.parametrize("rows,C", [(409600, 64), (25600, 1024), (6400, 2048), (102400, 128), (1000, 4)])
def test_batchnorm_reductions_large_and_repeatable(cuda, rows, C):
    """The BN statistics (conv-epilogue partials -> fold -> finalize) and the BN backward reduction at the model's
    large shapes: right against fp64, and bit-identical over repeated launches (fixed summation order)."""
    from boosted_detr_amd import kernels as k
    x = rnd(rows, C, seed=1) * 1.5 + 0.3
    dout = rnd(rows, C, seed=7)
    gamma, beta = 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
    xd_, dd_, gd_, bd_ = dev(x), dev(dout), dev(gamma), dev(beta)
    eps = 1.001e-5
    xd = x.double()
    m, v = xd.mean(0), xd.var(0, unbiased=False)
    # forward statistics through the many-partials path (one partial row per 32 rows, like the conv epilogue writes them)
    nparts = (rows + 31) // 32
    pad = nparts * 32 - rows
    xp = torch.cat([x, torch.zeros(pad, C)]) if pad else x
    psum = dev(xp.view(nparts, 32, C).sum(1)); psq = dev((xp * xp).view(nparts, 32, C).sum(1))
    first = None
    for it in range(12):
        mmd, mvd = dev(torch.zeros(C)), dev(torch.ones(C))
        mean, rstd = k.bn_stats(rows, C, (psum, psq, nparts), eps, 0.99, True, mmd, mvd, like=mmd)
        dx, dg, db, _ = k.bn_bwd(dd_, None, xd_, mean, rstd, gd_, True, False, beta=bd_)
        got = [t.clone() for t in (mean, rstd, mmd, mvd, dg, db)]
        if first is None:
            first = got
            close(mean, m, rtol=1e-5); close(rstd, 1 / torch.sqrt(v + eps), rtol=1e-4)
            xh = (xd - m) / torch.sqrt(v + eps)
            mask = (xh * gamma.double() + beta.double()) > 0
            g = dout.double() * mask
            close(db, g.sum(0), rtol=1e-4); close(dg, (g * xh).sum(0), rtol=1e-4)
        else:
            assert all(torch.equal(a, b) for a, b in zip(first, got)), it


def test_batchnorm_frozen(cuda):
    from boosted_detr_amd import kernels as k
    rows, C = 500, 128
    x, gamma, beta = rnd(rows, C, seed=1), 1 + 0.1 * rnd(C, seed=2), rnd(C, seed=3)
    mm, mv = rnd(C, seed=4), rnd(C, seed=5).abs() + 0.5
    mean, rstd = k.bn_stats_frozen(dev(mm), dev(mv), 1e-3)
    out = k.bn_apply(dev(x), mean, rstd, dev(gamma), dev(beta), None, True)
    xd = x.double().requires_grad_(True)
    ref = ((xd - mm.double()) / torch.sqrt(mv.double() + 1e-3) * gamma.double() + beta.double()).relu()
    close(out, ref)
    dout = rnd(rows, C, seed=7)
    ref.backward(dout.double())
    dx, dg, db, _ = k.bn_bwd(dev(dout), out, dev(x), mean, rstd, dev(gamma), True, True)
    close(dx, xd.grad)


@pytest.mark.parametrize("rows,D,rate", [(800, 256, 0.0), (100, 256, 0.1), (37, 64, 0.0), (50, 1024, 0.0)])
def test_add_dropout_layernorm(cuda, rows, D, rate):
    from boosted_detr_amd import kernels as k
    x, y = rnd(rows, D, seed=1), rnd(rows, D, seed=2)
    gamma, beta = 1 + 0.1 * rnd(D, seed=3), 0.1 * rnd(D, seed=4)
    out, mean, rstd = k.add_dropout_layernorm_fwd(dev(x), dev(y), dev(gamma), dev(beta), 1e-3, rate, 1234)
    if rate == 0.0:
        keep = torch.ones(rows, D, dtype=torch.float64)
    else:
        # recover the keep mask from a probe run: x=0, y=1, gamma=1, beta=0 -> h = keep/(1-rate)
        o2, m2, r2 = k.add_dropout_layernorm_fwd(dev(torch.zeros(rows, D)), dev(torch.ones(rows, D)), dev(torch.ones(D)),
                                                 dev(torch.zeros(D)), 1e-3, rate, 1234)
        h = o2.cpu().double() / r2.cpu().double()[:, None] + m2.cpu().double()[:, None]
        keep = (h > 0.5).double() / (1 - rate)
        frac = (keep > 0).double().mean().item()
        assert abs(frac - (1 - rate)) < 0.02, frac
    xd, yd = x.double().requires_grad_(True), y.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ref = F.layer_norm(xd + yd * keep, (D,), gd, bd, 1e-3)
    close(out, ref)
    dout = rnd(rows, D, seed=5)
    ref.backward(dout.double())
    dx, dy, dg, db = k.add_dropout_layernorm_bwd(dev(dout), dev(x), dev(y), dev(gamma), mean, rstd, rate, 1234)
    close(dx, xd.grad, rtol=1e-4)
    close(dy, yd.grad, rtol=1e-4)
    close(dg, gd.grad, rtol=1e-4)
    close(db, bd.grad, rtol=1e-4)


@pytest.mark.parametrize("rows,cols", [(64, 400), (33, 49), (10, 82), (5, 1050), (7, 3)])
def test_softmax(cuda, rows, cols):
    from boosted_detr_amd import kernels as k
    s, dp = rnd(rows, cols, seed=1) * 3, rnd(rows, cols, seed=2)
    scale = 0.17677669
    p = k.softmax_rows_fwd(dev(s), scale)
    sd = s.double().requires_grad_(True)
    ref = torch.softmax(sd * scale, -1)
    close(p, ref)
    ref.backward(dp.double())
    ds = k.softmax_rows_bwd(p, dev(dp), scale)
    close(ds, sd.grad, rtol=1e-4)


def test_maxpool(cuda):
    from boosted_detr_amd import kernels as k
    x = rnd(2, 15, 18, 64, seed=1).relu()
    y = k.maxpool_fwd(dev(x))
    xt = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    ref = F.max_pool2d(F.pad(xt, (1, 1, 1, 1)), 3, 2)
    close(y, ref.permute(0, 2, 3, 1), rtol=0, atol=0)
    dy = rnd(*ref.shape, seed=2).double()
    ref.backward(dy)
    dx = k.maxpool_bwd(dev(x), y, dev(dy.permute(0, 2, 3, 1).float()))
    m = (x > 0).double()     # ties at zero are masked by the producer's ReLU
    close(dx.cpu().double() * m, xt.grad.permute(0, 2, 3, 1) * m)


def test_activations(cuda):
    """Unit-scale inputs only (|x / 100| < 2 for the box sigmoid, |x| < 16 for the sigmoid): saturation, +-inf, NaN, -0.0 and the
    exp overflow points are tests/test_value_domain_gpu.py::test_pointwise_saturation_and_specials."""
    from boosted_detr_amd import kernels as k
    x, dy = rnd(1000, seed=1) * 50, rnd(1000, seed=2)
    xd = x.double().requires_grad_(True)
    ref = 3 * torch.sigmoid(xd / 100) - 1
    y = k.boxsigmoid_fwd(dev(x))
    close(y, ref, rtol=1e-6)
    ref.backward(dy.double())
    close(k.boxsigmoid_bwd(y, dev(dy)), xd.grad, rtol=1e-4)
    x2 = rnd(1000, seed=3) * 4
    x2d = x2.double().requires_grad_(True)
    r2 = torch.sigmoid(x2d)
    y2 = k.sigmoid_fwd(dev(x2))
    close(y2, r2, rtol=1e-6)
    r2.backward(dy.double())
    close(k.sigmoid_bwd(y2, dev(dy)), x2d.grad, rtol=1e-5)


def test_image_prep(cuda):
    from boosted_detr_amd import kernels as k
    from oracle import detr_oracle as O
    rng = np.random.default_rng(0)
    img = (rng.random((2, 40, 52, 3), dtype=np.float32) * 1.2 - 0.1).astype(np.float32)
    ref = O.Net(O.Config(image_size=(40, 52)), {}, torch.float32).image_prep(torch.from_numpy(img))
    out = k.image_prep(dev(img), 40, 52).cpu()
    assert torch.equal(out[..., :3], ref)            # integer pixel values: bit-exact
    assert (out[..., 3] == 0).all()
    ref2 = O.Net(O.Config(image_size=(32, 32)), {}, torch.float32).image_prep(torch.from_numpy(img))
    out2 = k.image_prep(dev(img), 32, 32).cpu()
    # resize: the uint8 truncation may flip by one unit where the interpolant lands within round-off of an integer
    diff = (out2[..., :3] - ref2).abs()
    assert diff.max() <= 1.0 and (diff > 0).double().mean() < 1e-3


def test_gemm_grouped_qkv(cuda):
    """Three projections with different inputs / weights / row counts in one launch (fwd and input grads)."""
    from boosted_detr_amd import kernels as k
    xs = [rnd(1600, 256, seed=1), rnd(6400, 256, seed=2), rnd(6400, 256, seed=3)]
    ws = [rnd(256, 256, seed=4, scale=1 / 16), rnd(256, 256, seed=5, scale=1 / 16), rnd(256, 256, seed=6, scale=1 / 16)]
    bs = [rnd(256, seed=7), rnd(256, seed=8), rnd(256, seed=9)]
    ys = k.linear_fwd_group([dev(x) for x in xs], [dev(w) for w in ws], [dev(b) for b in bs])
    for y, x, w, b in zip(ys, xs, ws, bs):
        close(y, x.double() @ w.double().T + b.double())
    dys = [rnd(1600, 256, seed=10), rnd(6400, 256, seed=11), rnd(6400, 256, seed=12)]
    dxs = k.linear_bwd_data_group([dev(d) for d in dys], [dev(w) for w in ws])
    for dx, dy, w in zip(dxs, dys, ws):
        close(dx, dy.double() @ w.double())


@pytest.mark.parametrize("policy", ["mixed", "split", "bf16x3", "fp32"])
@pytest.mark.parametrize("B,h,nq,nk", [(2, 8, 400, 400), (2, 8, 100, 400), (3, 8, 100, 100), (2, 8, 49, 49), (1, 4, 50, 49), (1, 8, 300, 1050)])
def test_fused_attention_fwd_bwd(cuda, B, h, nq, nk, policy):
    """csrc/attention.hip vs an fp64 reference of transformers.py:86-97 (incl. the [B,h,q,d] output layout), under every
    arithmetic policy: the forward is exact fp32 under 'mixed' / 'fp32', three split-f16 MFMA products under 'split' (fp32-grade),
    three split-bf16 ones under 'bf16x3'; the gradients are split-bf16 (2^-18 per product) except under 'fp32'."""
    from boosted_detr_amd import kernels as k
    D = h * 32
    Q, Kt, V = rnd(B, nq, D, seed=1), rnd(B, nk, D, seed=2), rnd(B, nk, D, seed=3)
    Q[0, 0] *= 6.0                                   # a spiky row: exercises the online-softmax rescale
    dO = rnd(B, h, nq, 32, seed=4)
    scale = 1.0 / np.sqrt(32.0)
    with k.gemm_precision(policy):
        o, lse = k.attention_fwd(dev(Q), dev(Kt), dev(V), h, scale)
    Qd, Kd, Vd = (t.double().requires_grad_(True) for t in (Q, Kt, V))
    Qh = Qd.view(B, nq, h, 32).permute(0, 2, 1, 3)
    Kh = Kd.view(B, nk, h, 32).permute(0, 2, 3, 1)
    Vh = Vd.view(B, nk, h, 32).permute(0, 2, 1, 3)
    s = (Qh @ Kh) * scale
    ref = torch.softmax(s, -1) @ Vh                                  # [B,h,q,32]
    fwd_tol = 5e-5 if policy == "bf16x3" else 1e-5
    close(o, ref, rtol=fwd_tol)
    close(lse, torch.logsumexp(s, -1), rtol=fwd_tol)
    ref.backward(dO.double())
    with k.gemm_precision(policy):
        dq, dk, dv = k.attention_bwd(dev(Q), dev(Kt), dev(V), o, dev(dO), lse, h, scale)
    # Gradients under split-bf16: dS = P (dP - D) cancels for a peaked row (the spiky query: P ~ one-hot, dP ~ D), so dS carries
    # the 2^-18 product error of dP relative to |dP|, not to |dS| - measured worst 8e-5 of max|dK| on these inputs (the convolutions'
    # gradient bar is 6e-5, the end-to-end bound of test_backward_arithmetic_in_isolation 2e-4); exact fp32 holds 5e-5
    bwd_tol = 5e-5 if policy == "fp32" else 2e-4
    close(dq, Qd.grad, rtol=bwd_tol)
    close(dk, Kd.grad, rtol=bwd_tol)
    close(dv, Vd.grad, rtol=bwd_tol)


@pytest.mark.parametrize("M,n", [(6400, 3), (1600, 2), (300, 4)])
def test_grouped_weight_gradients_in_one_split_k_launch(cuda, M, n):
    """bdetr_gemm_grouped with splitk > 1: the weight gradients of n Dense layers of one shape (256 x 256, M tokens) in ONE launch, slices
    adding with float atomics into zeroed / running-sum destinations."""
    from boosted_detr_amd import kernels as k
    dys = [rnd(M, 256, seed=10 + i) for i in range(n)]
    xs = [rnd(M, 256, seed=20 + i) for i in range(n)]
    base = [rnd(256, 256, seed=30 + i) if i == 0 else None for i in range(n)]            # the first destination holds a running sum
    dws = [dev(b) if b is not None else torch.empty(256, 256).cuda() for b in base]
    with k.gemm_precision("split"):
        k.linear_bwd_weight_group([dev(t) for t in dys], [dev(t) for t in xs], dws, [b is not None for b in base])
    for i in range(n):
        want = dys[i].double().T @ xs[i].double() + (base[i].double() if base[i] is not None else 0)
        close(dws[i], want, rtol=6e-5)
