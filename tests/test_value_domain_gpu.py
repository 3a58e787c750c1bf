"""Value-domain tests: the normalisation, softmax / attention, pointwise and optimiser kernels on ill-conditioned and extreme inputs
against fp64 (tests/_value_domain.py has the generators and the error models; tests/test_value_domain_cpu.py shows them sound).

The other kernel tests pin shapes; these pin VALUES: |mean| / sigma up to 1000, sigma down to 1e-3, constant, 1e-20, 1e15 and 1e19
channels / rows, saturated logits, attention scores up to 80 with the dominant key placed early and late.  Bars are error models
in u = 2^-24 stated next to each case; every test prints its worst measured `error / model` ratio (DESIGN.md "Value domain"
records them).  Shapes are the smallest that reach every code path named."""
import math

import numpy as np
import pytest
import torch

import _adamw_ref as R
import _value_domain as vd

pytestmark = pytest.mark.gpu
U, EPS = vd.U, 1.001e-5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def ratio(err, tol):
    """max err / tol; NaN / inf anywhere in err makes it inf."""
    q = np.asarray(err, np.float64) / np.asarray(tol, np.float64)
    return float("inf") if not np.isfinite(q).all() else float(q.max())


# =================================================================================================================================
# 1. BatchNorm
# =================================================================================================================================
def finalize(rows, C, parts):
    """bn_stats with momentum 0 into zeroed moving statistics (no Bessel factor): (mean, rstd, the kernel's own variance)."""
    from boosted_detr_amd import kernels as k
    mm, mv = torch.zeros(C).cuda(), torch.zeros(C).cuda()
    mean, rstd = k.bn_stats(rows, C, parts, EPS, 0.0, False, mm, mv, like=mm)
    assert torch.equal(mm, mean)
    return mean, rstd, mv


def check_stats(label, x, mean, rstd, var, Rc, names=None):
    """The statistics laws against fp64 moments of the fp32 data `x` [rows, C] (R = Rc); returns max |dvar| / (u (m^2 + s^2))."""
    m64, v64 = vd.moments64(x)
    mean, rstd, var = host(mean), host(rstd), host(var)
    bm, bv = vd.bn_bounds(m64, v64, Rc)
    assert not np.isnan(mean).any() and not np.isnan(var).any(), (label, "NaN statistics")
    assert np.isfinite(rstd).all() and (rstd > 0).all() and (rstd <= (1 + 2 * U) / math.sqrt(EPS)).all(), (label, rstd.min(), rstd.max())
    assert (var >= 0).all(), (label, "negative variance", var.min())
    em, ev, er = np.abs(mean - m64), np.abs(var - v64), np.abs(rstd - 1 / np.sqrt(v64 + EPS))
    worst = ratio(ev, U * (m64 ** 2 + v64) + vd.TINY)
    print("%s: max |dvar| / (u (m^2 + s^2)) = %.2f (bound R + 2 = %d), |dmean| / bound %.3f, |drstd| / bound %.3f"
          % (label, worst, Rc + 2, ratio(em, bm), ratio(er, vd.rstd_bound(v64, EPS, bv))))
    bad = lambda e, b: [(c, names[c] if names else "", float(e[c]), float(b[c])) for c in np.nonzero(~(e <= b))[0]]
    assert (em <= bm).all(), (label, "mean", bad(em, bm))
    assert (ev <= bv).all(), (label, "var", bad(ev, bv))
    assert (er <= vd.rstd_bound(v64, EPS, bv)).all(), (label, "rstd", bad(er, vd.rstd_bound(v64, EPS, bv)))
    if names:
        tiny = [c for c, n in enumerate(names) if n == "tiny"]
        assert (np.abs(rstd[tiny] * math.sqrt(EPS) - 1) <= 2 * U).all()          # squares underflow: var = 0, rstd = 1 / sqrt(eps) to u
    return worst


# R of colstats (csrc/norm.hip colreduce2_kernel, C = 64 -> 16 column threads x 16 row phases, 64-row chunks): a thread adds its 4
# rows in turn, then a 4-level LDS tree: 8 fp32 additions on the longest chain; the chunk partials are folded in fp64
R_COLSTATS = 8


@pytest.mark.parametrize("rows", [98, 800])
def test_bn_colstats_statistics_apply_and_backward(cuda, rows):
    """(a) colstats -> bn_stats per regime, then bn_apply (with / without residual and ReLU) and bn_bwd (mask from `out` and
    recomputed) against fp64 WITH THE KERNEL'S OWN mean and rstd.  Statistics: |dmean| <= (R+2) u (|m|+s), |dvar| <= (R+2) u (m^2+s^2),
    R = 8.  Apply / backward: project bar + 8 u r |gamma| per channel.  Constant channels: no NaN (raw variance is negative for
    1000.1 - the clamp), finite gradients, out == beta (+ residual, ReLU) bit for bit where the fp32 sums are exact (0.5, -1024, 0)
    and within (R+2) u |m| rstd |gamma| of it otherwise - the mean of a non-dyadic constant carries the moment scheme's error, and
    rstd = 1 / sqrt(eps) = 316 magnifies it (DESIGN.md "Value domain").
    measured on MI355X, 2026-10-21: max |dvar| / (u (m^2 + s^2)) 1.98 (98 rows) / 1.08 (800), bound 10; |dmean| 0.13 and |drstd| 0.27
    of their bounds; bn_apply 0.006 and bn_bwd 0.001 of their bars."""
    from boosted_detr_amd import kernels as k
    C = 64
    x, names = vd.bn_input(rows, C, seed=11)
    xd = dev(x)
    mean, rstd, var = finalize(rows, C, k.colstats(xd))
    check_stats("colstats rows=%d" % rows, x, mean, rstd, var, R_COLSTATS, names)
    rng = np.random.default_rng(12)
    gamma, beta = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32)
    resid, dout = rng.standard_normal((rows, C)).astype(np.float32), rng.standard_normal((rows, C)).astype(np.float32)
    mk, rk = host(mean), host(rstd)
    m64, v64 = vd.moments64(x)
    gd, bd = gamma.astype(np.float64), beta.astype(np.float64)
    xh = (x.astype(np.float64) - mk) * rk
    worst_f = worst_b = 0.0
    for res in (False, True):
        for relu in (False, True):
            out = k.bn_apply(xd, mean, rstd, dev(gamma), dev(beta), dev(resid) if res else None, relu)
            ref = xh * gd + bd + (resid if res else 0.0)
            ref = np.maximum(ref, 0) if relu else ref
            o = host(out)
            worst_f = max(worst_f, ratio(np.abs(o - ref).max(0), vd.bn_apply_tol(ref, m64, v64, gamma, EPS)))
            for c, n in enumerate(names):
                if n != "const":
                    continue
                want = (beta[c] + resid[:, c]).astype(np.float32) if res else np.full(rows, beta[c], np.float32)
                want = np.maximum(want, np.float32(0)) if relu else want
                if float(x[0, c]) in vd.BN_DYADIC:
                    assert np.array_equal(out[:, c].cpu().numpy(), want), ("constant channel", float(x[0, c]), res, relu)
                else:
                    lim = (R_COLSTATS + 2) * U * abs(m64[c]) * rk[c] * abs(gd[c]) + 2 * U * (abs(bd[c]) + (np.abs(resid[:, c]).max() if res else 0))
                    assert np.abs(o[:, c] - want).max() <= lim, ("constant channel", float(x[0, c]), np.abs(o[:, c] - want).max(), lim)
            # backward: the ReLU mask is `out`'s sign, an input of the kernel
            g = dout.astype(np.float64) * ((o > 0) if relu else 1.0)
            dbeta, dgamma = g.sum(0), (g * xh).sum(0)
            dx = (g - dbeta / rows - xh * dgamma / rows) * rk * gd
            widen = vd.BWD_BAR + 8 * U * np.abs(m64) / np.sqrt(v64 + EPS)
            got = k.bn_bwd(dev(dout), out if relu else None, xd, mean, rstd, dev(gamma), relu, False, want_residual_grad=res)
            assert all(torch.isfinite(t).all() for t in got if t is not None)
            worst_b = max(worst_b, ratio(np.abs(host(got[0]) - dx).max(0), widen * np.abs(dx).max(0) + vd.TINY),
                          ratio(np.abs(host(got[1]) - dgamma), widen * np.abs(g * xh).sum(0) + vd.TINY),
                          ratio(np.abs(host(got[2]) - dbeta), widen * np.abs(g).sum(0) + vd.TINY))
            if res:
                assert np.array_equal(host(got[3]), g)
            if relu and not res:           # the mask recomputed from x rounds as the forward did: identical results
                again = k.bn_bwd(dev(dout), None, xd, mean, rstd, dev(gamma), True, False, beta=dev(beta))
                assert all(torch.equal(a, b) for a, b in zip(got[:3], again[:3]))
    print("bn_apply rows=%d: worst error / (project bar + 8 u r |gamma|) = %.3f; bn_bwd: %.3f" % (rows, worst_f, worst_b))
    assert worst_f <= 1 and worst_b <= 1


# R of the hand-made partials: 31 additions inside a 32-row partial.  nparts = 300 > 4 x 64 takes fold_partials2_kernel, whose 8-phase
# fp32 sum adds 7 more; bn_finalize_kernel then folds the 64 rows in fp64.
R_HAND_MADE = 31 + 7


@pytest.mark.parametrize("start", [0, 5])
def test_bn_stats_from_hand_made_partials(cuda, start):
    """(b) 300 fp32 partials of 32 rows (rows 9600, C 8: the regimes at two rotations) through fold_partials2 + bn_finalize.
    measured on MI355X, 2026-10-21: max |dvar| / (u (m^2 + s^2)) 0.22 (rotation 0) / 0.75 (rotation 5), bound 40: the 32-row
    partials carry the error, not the fold."""
    from boosted_detr_amd import _lib
    rows, C, nparts = 9600, 8, 300
    assert nparts > 4 * _lib.lib().bdetr_bn_stats_fold_rows()
    x, names = vd.bn_input(rows, C, seed=13, start=start)
    xt = torch.from_numpy(x)
    parts = (xt.view(nparts, 32, C).sum(1).cuda(), (xt * xt).view(nparts, 32, C).sum(1).cuda(), nparts)
    mean, rstd, var = finalize(rows, C, parts)
    w = check_stats("hand-made partials start=%d R=%d" % (start, R_HAND_MADE), x, mean, rstd, var, R_HAND_MADE, names)
    print("VALUE_DOMAIN_RATIO %.3f" % w)


# R of bn_rows_stats (csrc/groupnorm_rows.hip group_colsum2): 64 row phases, a thread adds ceil(rows / 64) rows in fp32, the 64 phase
# partials are folded in fp64: R = 2 at 65 rows, 1 at 7
@pytest.mark.parametrize("G,Rg,C", [(2, 65, 48), (4, 7, 64)])
def test_bn_rows_statistics_apply_backward_and_no_leak_between_groups(cuda, G, Rg, C):
    """(f) Even groups carry the regimes, odd groups are ordinary randn: every group is held to the bound of ITS OWN moments, so a
    partial sum that straddled a group boundary (means of 1000 next to means of 0) fails the ordinary group by orders of magnitude.
    measured on MI355X, 2026-10-21: max |dvar| / (u (m^2 + s^2)) 0.83 at (2,65,48) (bound 4), 1.06 at (4,7,64) (bound 3); |drstd| 0.53
    of its bound; bn_rows_apply 0.007 and bn_rows_bwd 0.003 of their bars."""
    from boosted_detr_amd import kernels as k
    Rc = -(-Rg // 64)
    xs, allnames = [], []
    for g in range(G):
        if g % 2 == 0:
            xg, names = vd.bn_input(Rg, C, seed=20 + g, start=3 * g)
        else:
            xg, names = np.random.default_rng(20 + g).standard_normal((Rg, C)).astype(np.float32), None
        xs.append(xg); allnames.append(names)
    x = np.concatenate(xs)
    xd = dev(x)
    mean, rstd, var = k.bn_rows_stats(xd, G, EPS)
    for g in range(G):
        check_stats("bn_rows_stats (%d,%d,%d) group %d%s" % (G, Rg, C, g, "" if g % 2 == 0 else " (ordinary)"), xs[g], mean[g], rstd[g], var[g], Rc, allnames[g])
    rng = np.random.default_rng(21)
    gamma, beta = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32)
    dout = rng.standard_normal((G * Rg, C)).astype(np.float32)
    out = host(k.bn_rows_apply(xd, G, mean, rstd, dev(gamma), dev(beta)))
    dx, dgamma, dbeta = (host(t) for t in k.bn_rows_bwd(dev(dout), xd, G, mean, rstd, dev(gamma), False))
    assert np.isfinite(dx).all() and np.isfinite(dgamma).all() and np.isfinite(dbeta).all()
    gd, bd = gamma.astype(np.float64), beta.astype(np.float64)
    worst_f = worst_b = 0.0
    ref_dg, ref_db, tol_dg, tol_db = np.zeros(C), np.zeros(C), np.zeros(C), np.zeros(C)
    for g in range(G):
        sl = slice(g * Rg, (g + 1) * Rg)
        mk, rk = host(mean[g]), host(rstd[g])
        m64, v64 = vd.moments64(xs[g])
        xh = (xs[g].astype(np.float64) - mk) * rk
        ref = xh * gd + bd
        worst_f = max(worst_f, ratio(np.abs(out[sl] - ref).max(0), vd.bn_apply_tol(ref, m64, v64, gamma, EPS)))
        gg = dout[sl].astype(np.float64)
        db, dg = gg.sum(0), (gg * xh).sum(0)
        rdx = (gg - db / Rg - xh * dg / Rg) * rk * gd
        widen = vd.BWD_BAR + 8 * U * np.abs(m64) / np.sqrt(v64 + EPS)
        worst_b = max(worst_b, ratio(np.abs(dx[sl] - rdx).max(0), widen * np.abs(rdx).max(0) + vd.TINY))
        ref_dg += dg; ref_db += db; tol_dg += widen * np.abs(gg * xh).sum(0); tol_db += widen * np.abs(gg).sum(0)
        if allnames[g]:
            for c, n in enumerate(allnames[g]):
                if n == "const" and float(xs[g][0, c]) in vd.BN_DYADIC:
                    assert np.array_equal(out[sl, c].astype(np.float32), np.full(Rg, beta[c], np.float32))
    worst_b = max(worst_b, ratio(np.abs(dgamma - ref_dg), tol_dg + vd.TINY), ratio(np.abs(dbeta - ref_db), tol_db + vd.TINY))
    print("bn_rows_apply (%d,%d,%d): worst error / bar %.3f; bn_rows_bwd: %.3f" % (G, Rg, C, worst_f, worst_b))
    assert worst_f <= 1 and worst_b <= 1


@pytest.mark.parametrize("producer", ["partials", "colstats"])
def test_bn_huge_channel_raises_the_guard_and_keeps_the_moving_statistics(cuda, producer):
    """1e19 channels: their squares overflow fp32, the statistics are not finite - with the range guard active bn_stats must raise
    the overflow flag and leave moving_mean / moving_var bit-unchanged, all channels.  bn_finalize_kernel raises and reads the flag
    in ONE launch, a workgroup (one wave finalising) per 32 channels: the channels of a workgroup that holds a non-finite channel
    are kept on every run, a workgroup without one is not ordered against the raise (DESIGN.md "Value domain": a limit of the
    kernel, not exercised here).  So every finalising workgroup gets a huge channel: channel 5 at C = 8 (hand-made partials
    through fold_partials2, one workgroup) and channels 5 and 37 at C = 64 (colstats, two workgroups).  A launch behind it, the
    flag still up, touches nothing either; with the flag cleared and no huge channel every channel is updated."""
    from boosted_detr_amd import kernels as k
    rows, C = (9600, 8) if producer == "partials" else (98, 64)
    huge = list(range(5, C, 32))
    x, _ = vd.bn_input(rows, C, seed=14)
    x[:, huge] = (vd.BN_HUGE * np.random.default_rng(15).standard_normal((rows, len(huge)))).astype(np.float32)
    assert np.isfinite(x).all()

    def parts(a):
        if producer == "colstats":
            return k.colstats(dev(a))
        t = torch.from_numpy(a)
        return t.view(300, 32, C).sum(1).cuda(), (t * t).view(300, 32, C).sum(1).cuda(), 300

    k.read_and_clear_overflow()
    was_active = k._GUARD_ACTIVE[0]
    k.set_guard_active(True)
    mm0, mv0 = torch.randn(C, generator=torch.Generator().manual_seed(1)), torch.rand(C, generator=torch.Generator().manual_seed(2)) + 0.5
    mm, mv = mm0.cuda(), mv0.cuda()
    try:
        mean, rstd = k.bn_stats(rows, C, parts(x), EPS, 0.99, True, mm, mv, like=mm)
        torch.cuda.synchronize()
        assert int(k.overflow_flag().item()) == 1, "the guard did not rise"
        assert not torch.isnan(mean).any()
        assert torch.equal(mm.cpu(), mm0) and torch.equal(mv.cpu(), mv0), "moving statistics touched while the guard is up"
        k.bn_stats(rows, C, parts(np.ones_like(x)), EPS, 0.99, True, mm, mv, like=mm)          # the flag is still up: nothing moves
        assert torch.equal(mm.cpu(), mm0) and torch.equal(mv.cpu(), mv0)
        assert k.read_and_clear_overflow() is True
        x[:, huge] = 1.0                   # the same launch without the huge channels updates every channel
        k.bn_stats(rows, C, parts(x), EPS, 0.99, True, mm, mv, like=mm)
        assert k.read_and_clear_overflow() is False and not (mm.cpu() == mm0).any()
    finally:
        k.overflow_flag().zero_()
        k.set_guard_active(was_active)


# R of the convolution epilogues: one partial row per bm / wm = 32 or 64 output rows of a tile (igemm.hip stat_chunks: tiles_i x WM
# partial rows); at most 64 fp32 additions whichever tile the chooser takes, the 98 rows give < 4 x 64 partials: fp64 from there on
R_CONV = 64
CONV_GEOM = (2, 7, 7, 64, 64)


def conv_case(rmax=None):
    """A 1x1 convolution whose OUTPUT channel k follows regime k: input channel 0 is constant 1, so w[k, 0] is the channel's offset;
    the other 63 input channels are randn and w[k, 1:] a random direction of norm sigma_k.  (x, w, bias, names)"""
    N, H, W, Cc, K = CONV_GEOM
    rng = np.random.default_rng(16)
    names, mean, sigma = vd.bn_targets(K, 0, rmax)
    x = rng.standard_normal((N, H, W, Cc)).astype(np.float32)
    x[..., 0] = 1.0
    w = rng.standard_normal((K, Cc))
    w[:, 1:] *= (sigma / np.linalg.norm(w[:, 1:], axis=1))[:, None]
    w[:, 0] = mean
    return x, w.reshape(K, 1, 1, Cc).astype(np.float32), np.zeros(K, np.float32), names


def test_bn_statistics_from_the_fp32_conv_epilogue(cuda):
    """(d) conv2d_fwd(want_stats=True) on the fp32 policy: the epilogue's partials against fp64 moments of the y the launch wrote
    (R = 64), y itself against the fp64 convolution at the project bar.
    measured on MI355X, 2026-10-21: max |dvar| / (u (m^2 + s^2)) 4.29 (bound 66); y 0.043 of its bar."""
    from boosted_detr_amd import kernels as k
    N, H, W, Cc, K = CONV_GEOM
    x, w, b, names = conv_case()
    g = k.ConvGeom(N, H, W, Cc, K, 1, 1, 1, 0)
    with k.gemm_precision("fp32"):
        y, parts = k.conv2d_fwd(dev(x), dev(w), dev(b), g, 0, want_stats=True)
    yh = host(y).reshape(-1, K)
    ref = x.reshape(-1, Cc).astype(np.float64) @ w.reshape(K, Cc).astype(np.float64).T
    mag = np.abs(x.reshape(-1, Cc).astype(np.float64)) @ np.abs(w.reshape(K, Cc).astype(np.float64)).T
    q = ratio(np.abs(yh - ref).max(0), vd.FWD_BAR * mag.max(0) + vd.TINY)
    print("conv2d_fwd fp32 y: worst error / (2e-5 max sum |x w|) per channel = %.3f" % q)
    assert q <= 1
    mean, rstd, var = finalize(N * H * W, K, parts)
    check_stats("fp32 conv epilogue", yh.astype(np.float32), mean, rstd, var, R_CONV, names)


def test_bn_statistics_from_the_p16_conv_epilogue(cuda):
    """(e) The same geometry through p16_conv2d_fwd (f16-pair operands), regimes of r <= 100 (the forward weight copy holds 2^8 w
    in f16: offsets beyond 255 leave its range).  Quantisation (p16.h): an operand is hi + lo with 11 significant bits each, 2^-22
    relative (2^-25 absolute below 2^-3, where lo is subnormal), the weight copy likewise at 2^-8 of those magnitudes, and the product
    drops lo x lo: 3 x 2^-22 x sum |x w| on y, added to the project bar.  The statistics are held to the moments of the y the launch
    wrote, R = 64, so the operands' quantisation does not enter their bound.
    measured on MI355X, 2026-10-21: max |dvar| / (u (m^2 + s^2)) 5.74 (bound 66); y 0.018 of its bar."""
    from boosted_detr_amd import kernels as k
    N, H, W, Cc, K = CONV_GEOM
    x, w, b, names = conv_case(rmax=100)
    g = k.ConvGeom(N, H, W, Cc, K, 1, 1, 1, 0)
    assert k.p16_supported(g)
    k.read_and_clear_overflow()
    xf, _ = k.p16_pack(dev(x), want_bf16=False)
    wf, _ = k.p16_pack_conv_weights(dev(w), want_bwd=False)
    y, parts = k.p16_conv2d_fwd(xf, wf, dev(b), g, 0, want_stats=True)
    assert k.read_and_clear_overflow() is False
    yh = host(y).reshape(-1, K)
    X, Wm = x.reshape(-1, Cc).astype(np.float64), w.reshape(K, Cc).astype(np.float64)
    mag = np.abs(X) @ np.abs(Wm).T
    # a weight below the f16 copy's subnormal spacing (2^-24 / 2^8) flushes: absolute 2^-33 per weight x sum |x|
    tol = (vd.FWD_BAR + 3 * 2.0 ** -22) * mag.max(0) + 2.0 ** -33 * np.abs(X).sum(1).max()
    q = ratio(np.abs(yh - X @ Wm.T).max(0), tol)
    print("p16_conv2d_fwd y: worst error / (project bar + 3 x 2^-22 quantisation) = %.3f" % q)
    assert q <= 1
    mean, rstd, var = finalize(N * H * W, K, parts)
    check_stats("p16 conv epilogue", yh.astype(np.float32), mean, rstd, var, R_CONV, None)


# =================================================================================================================================
# 2. LayerNorm family
# =================================================================================================================================
LN_EPS = 1e-3


def ln_params(D, seed):
    rng = np.random.default_rng(seed)
    return (1 + 0.1 * rng.standard_normal(D)).astype(np.float32), (0.1 * rng.standard_normal(D)).astype(np.float32)


def check_ln_rows(label, names, out, rstd, ref, h, gamma, exact, bar=vd.FWD_BAR):
    """Forward bars per row; constant rows: rstd = 1 / sqrt(eps) (where the kernel returns rstd), out == `exact` (beta, through the
    activation) bit for bit where the row sum is exact (const2)."""
    assert np.isfinite(out).all(), (label, "non-finite output")
    tol = vd.ln_fwd_tol(ref, h, gamma, LN_EPS, bar)
    err = np.abs(out - ref).max(-1)
    assert (err <= tol).all(), (label, [(n, e / t) for n, e, t in zip(names, err, tol) if not e <= t])
    for i, n in enumerate(names):
        if n in ("const", "const2", "tiny") and rstd is not None:
            assert abs(rstd[i] * math.sqrt(LN_EPS) - 1) <= 4 * U, (label, n, rstd[i])
        if n == "const2":
            assert np.array_equal(out[i].astype(np.float32), exact), (label, "constant row is not beta")
    return ratio(err, tol)


@pytest.mark.parametrize("rows,D,start", [(37, 64, 0), (5, 1024, 0), (5, 1024, 3)])
def test_add_dropout_layernorm_value_domain(cuda, rows, D, start):
    """add_dropout_layernorm_fwd / bwd at rate 0: rows of r in {0, 10, 100, 1000}, constant (3.3 and -4), 1e-20 and 1e15 (five rows
    at D = 1024: two rotations cover the eight regimes).  Forward: project bar + (2 + log2 D) u r max|gamma| per row; backward: that
    factor on the 1e-4 bar.  r uses sqrt(var + eps) as the yardstick, so the constant row 3.3 - whose fp32 row sum rounds - is held
    to the same law; -4.0 sums exactly and must give beta bit for bit.  A one-pass fp32 variance misses the r = 1000 row (by 44 to
    85 bars when add_drop_ln_fwd_kernel is so mutated).
    measured on MI355X, 2026-10-21: forward 0.117 of the bar at (37,64), 0.012 / 0.006 at (5,1024); backward 0.026 / 0.005 / 0.004."""
    from boosted_detr_amd import kernels as k
    x, names = vd.ln_input(rows, D, seed=30, start=start)
    rng = np.random.default_rng(31)
    y = np.zeros((rows, D), np.float32)
    for i, n in enumerate(names):
        if n == "r0":
            y[i] = 0.5 * rng.standard_normal(D)          # the Add is exercised on the ordinary rows; x + y is exact elsewhere
    gamma, beta = ln_params(D, 32)
    dout = rng.standard_normal((rows, D)).astype(np.float32)
    out, mean, rstd = k.add_dropout_layernorm_fwd(dev(x), dev(y), dev(gamma), dev(beta), LN_EPS, 0.0, 0)
    h = x.astype(np.float64) + y.astype(np.float64)
    ref, m64, rstd64, xh = vd.ln_ref64(h, gamma, beta, LN_EPS)
    wf = check_ln_rows("add_dropout_layernorm_fwd", names, host(out), host(rstd), ref, h, gamma, beta)
    dx, dy, dg, db = (host(t) for t in k.add_dropout_layernorm_bwd(dev(dout), dev(x), dev(y), dev(gamma), mean, rstd, 0.0, 0))
    assert all(np.isfinite(t).all() for t in (dx, dy, dg, db))
    dd, gd = dout.astype(np.float64), gamma.astype(np.float64)
    rdh, rdg, rdb = vd.ln_bwd64(dd, xh, rstd64, gd)
    f = vd.ln_bwd_factor(h, gamma, LN_EPS)
    tol_rows = (vd.BWD_BAR + f) * np.abs(rdh).max(-1) + vd.TINY
    wb = max(ratio(np.abs(dx - rdh).max(-1), tol_rows), ratio(np.abs(dy - rdh).max(-1), tol_rows),
             ratio(np.abs(dg - rdg), ((vd.BWD_BAR + f)[:, None] * np.abs(dd) * np.maximum(np.abs(xh), 1)).sum(0)),
             ratio(np.abs(db - rdb), vd.BWD_BAR * np.abs(dd).sum(0)))
    print("add_dropout_layernorm (%d,%d) start %d: forward error / bar %.3f, backward %.3f" % (rows, D, start, wf, wb))
    assert wb <= 1


@pytest.mark.parametrize("slope", [0.01, 1.0])
def test_layernorm_act_value_domain(cuda, slope):
    """layernorm_act / layernorm_act_bwd at C = 29 of 32 stored columns (the padding holds junk the kernel must not read), 19 rows.
    Same bars as above.  The leaky slope's branch is taken from the sign of gamma xhat + beta: the generator keeps every
    reference value further from zero than two forward bars, so a kernel within one bar takes the branch fp64 takes.  The constant
    row -4.0 must give leaky(beta) bit for bit at either slope.  The kernel returns no rstd, so rstd = 1 / sqrt(eps) on constant rows
    is seen only through the output bar here.
    measured on MI355X, 2026-10-21: forward 0.096 of the bar at either slope; backward 0.059 (slope 0.01) / 0.030 (slope 1)."""
    from boosted_detr_amd import kernels as k
    rows, C, ld = 19, 29, 32
    xc, names = vd.ln_input(rows, C, seed=40)
    gamma, beta = ln_params(C, 41)
    beta = (np.sign(beta) * (0.05 + np.abs(beta))).astype(np.float32)          # a constant row gives beta: keep it off the kink
    x = np.full((rows, ld), 7.0e3, np.float32)
    x[:, :C] = xc
    dout = np.random.default_rng(42).standard_normal((rows, ld)).astype(np.float32)
    v, _, rstd64, xh = vd.ln_ref64(xc, gamma, beta, LN_EPS)
    tol = vd.ln_fwd_tol(v, xc, gamma, LN_EPS)
    assert (np.abs(v).min(-1) > 2 * tol).all(), "a reference value sits on the leaky kink: pick another seed"
    ref = np.where(v >= 0, v, v * slope)
    out = host(k.layernorm_act(dev(x), C, dev(gamma), dev(beta), LN_EPS, slope))
    assert out.shape == (rows, ld) and (out[:, C:] == 0).all()
    leaky_beta = np.where(beta >= 0, beta, beta * np.float32(slope)).astype(np.float32)          # the kernel's own fp32 product
    wf = check_ln_rows("layernorm_act", names, out[:, :C], None, ref, xc, gamma, leaky_beta)
    dx, dg, db = (host(t) for t in k.layernorm_act_bwd(dev(x), C, dev(gamma), dev(beta), LN_EPS, slope, dev(dout)))
    assert np.isfinite(dx).all() and np.isfinite(dg).all() and np.isfinite(db).all() and (dx[:, C:] == 0).all()
    gp = dout[:, :C].astype(np.float64) * np.where(v >= 0, 1.0, slope)
    rdh, rdg, rdb = vd.ln_bwd64(gp, xh, rstd64, gamma.astype(np.float64))
    f = vd.ln_bwd_factor(xc, gamma, LN_EPS)
    wb = max(ratio(np.abs(dx[:, :C] - rdh).max(-1), (vd.BWD_BAR + f) * np.abs(rdh).max(-1) + vd.TINY),
             ratio(np.abs(dg - rdg), ((vd.BWD_BAR + f)[:, None] * np.abs(gp) * np.maximum(np.abs(xh), 1)).sum(0)),
             ratio(np.abs(db - rdb), vd.BWD_BAR * np.abs(gp).sum(0)))
    print("layernorm_act slope %g: forward error / bar %.3f, backward %.3f" % (slope, wf, wb))
    assert wb <= 1


ROW_FWD, ROW_BWD = 3e-5, 2e-4          # the row chain's project bars (tests/test_rowchain_gpu.py: f16-pair forward, bf16-pair gradient products)


@pytest.mark.parametrize("nstages", [1, 3])
def test_rowchain_value_domain(cuda, nstages):
    """rowchain_fwd / bwd at M = 33, the extreme rows entering through the RESIDUAL operand (ctx is zero on the constant and 1e-20
    rows and the output projection's bias is zero, so those rows reach the LayerNorm as generated).  Forward against the fp64
    chain: pre1 to 3e-5 max|ctx Wo^T| + 2u |row|; x1 to the project bar + (2 + log2 256) u r max|gamma| + the projection's own
    3e-5 max|ctx Wo^T| through rstd |gamma|; h, pre2, x2 to the project bar + 4 x that row's x1 bar (two Dense layers of spectral
    norm <= 2 each: N(0, 1/D) square matrices).  Backward against an fp64 restatement FROM THE TENSORS THE BACKWARD KERNEL WAS
    GIVEN (pre1, h, pre2 and the saved means / rstds; the ReLU mask is h's sign): (2e-4 + 4 (2 + log2 256) u r max|gamma|) x max|ref|
    per row.  Constant row -4.0: x1 == beta1 bit for bit; rstd = 1 / sqrt(eps) on constant and 1e-20 rows; everything finite.
    measured on MI355X, 2026-10-21 (error / bar): pre1 0.133, x1 0.094, h 0.027, pre2 0.032, x2 0.018; backward dctx 0.042, dres 0.028,
    G1 0.037, the seven parameter vectors <= 0.045."""
    from boosted_detr_amd import _lib, kernels as k
    from test_rowchain_gpu import D, make_params
    M = 33
    p = {kk: v.numpy().astype(np.float32) for kk, v in make_params(10).items()}
    p["bo"] = np.zeros(D, np.float32)
    resid, rnames = vd.ln_input(M, D, seed=33)
    rng = np.random.default_rng(34)
    ctx = rng.standard_normal((M, D)).astype(np.float32)
    for i, n in enumerate(rnames):
        if n in ("const", "const2", "tiny"):
            ctx[i] = 0
    dout = rng.standard_normal((M, D)).astype(np.float32)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n = int(_lib.lib().bdetr_rowchain_pack_elems())
    wnames = ["Wo", "W1", "W2"][:nstages]
    wdev = {w: T(p[w]) for w in wnames}
    fwd = {w: torch.empty(n, device="cuda") for w in wnames}
    bwd = {w: torch.empty(n, device="cuda") for w in wnames}
    k.rowchain_pack_weights(torch.tensor([[wdev[w].data_ptr(), fwd[w].data_ptr(), bwd[w].data_ptr()] for w in wnames], dtype=torch.int64).cuda())
    biases = [T(p[b]) for b in ["bo", "b1", "b2"][:nstages]]
    ln1, ln2 = (T(p["g1"]), T(p["be1"])), ((T(p["g2"]), T(p["be2"])) if nstages == 3 else None)
    saved = k.rowchain_fwd(T(ctx), T(resid), [fwd[w] for w in wnames], biases, ln1, ln2, LN_EPS, 0.0, 0, 0, None)
    S = {kk: host(v) for kk, v in saved.items()}
    assert all(np.isfinite(v).all() for v in S.values()), [kk for kk, v in S.items() if not np.isfinite(v).all()]
    q = {kk: v.astype(np.float64) for kk, v in p.items()}
    # ---- forward, fp64 from the fp32 inputs
    a = ctx.astype(np.float64) @ q["Wo"].T
    pre1 = resid.astype(np.float64) + a
    x1, _, rstd1, _ = vd.ln_ref64(pre1, q["g1"], q["be1"], LN_EPS)
    delta = (2 + math.log2(D)) * U * vd.ln_r(pre1, LN_EPS) * np.abs(q["g1"]).max()
    amax = np.abs(a).max()
    worst = {"pre1": ratio(np.abs(S["pre1"] - pre1).max(-1), ROW_FWD * amax + 2 * U * np.abs(pre1).max(-1))}
    e1 = ROW_FWD * np.abs(x1).max() + delta + ROW_FWD * amax * rstd1 * np.abs(q["g1"]).max()
    worst["x1"] = ratio(np.abs(S["x1"] - x1).max(-1), e1)
    worst["rstd1"] = ratio(np.abs(S["rstd1"] / rstd1 - 1), ROW_FWD * np.maximum(1, amax * rstd1) + delta + 4 * U)
    for i, nm in enumerate(rnames):
        if nm in ("const", "const2", "tiny"):
            assert abs(S["rstd1"][i] * math.sqrt(LN_EPS) - 1) <= 4 * U, (nm, S["rstd1"][i])
        if nm == "const2":
            assert np.array_equal(S["x1"][i].astype(np.float32), p["be1"]), "constant row is not beta"
    if nstages == 3:
        h = np.maximum(x1 @ q["W1"].T + q["b1"], 0)
        pre2 = x1 + h @ q["W2"].T + q["b2"]
        x2, _, rstd2, _ = vd.ln_ref64(pre2, q["g2"], q["be2"], LN_EPS)
        for key, ref, gain in (("h", h, 1.0), ("pre2", pre2, 1.0), ("x2", x2, np.maximum(1, rstd2 * np.abs(q["g2"]).max()))):
            worst[key] = ratio(np.abs(S[key] - ref).max(-1), ROW_FWD * np.abs(ref).max() + 4 * e1 * gain)
    # ---- backward, fp64 from the tensors the backward kernel reads
    gammas = (ln1[0],) + ((ln2[0],) if nstages == 3 else ())
    dctx, dres, G, partials, nparts = k.rowchain_bwd(T(dout), saved, [bwd[w] for w in wnames], gammas, 0.0, 0, 0, None)
    vec = [torch.zeros(D, device="cuda") for _ in range(7)]
    k.rowchain_reduce(partials, nparts, vec if nstages == 3 else [None] * 4 + vec[4:], [0] * 7)
    wrow = ROW_BWD + 4 * delta
    dd = dout.astype(np.float64)
    want_vec = {}
    if nstages == 3:
        xh2 = (S["pre2"] - S["mean2"][:, None]) * S["rstd2"][:, None]
        dpre2, want_vec[0], want_vec[1] = vd.ln_bwd64(dd, xh2, S["rstd2"], q["g2"])
        dhid = (dpre2 @ q["W2"]) * (S["h"] > 0)
        dx1 = dpre2 + dhid @ q["W1"]
        want_vec[2], want_vec[3] = dpre2.sum(0), dhid.sum(0)
        terms = {0: dd * xh2, 1: dd, 2: dpre2, 3: dhid}
    else:
        dx1, terms = dd, {}
    xh1 = (S["pre1"] - S["mean1"][:, None]) * S["rstd1"][:, None]
    dpre1, want_vec[4], want_vec[5] = vd.ln_bwd64(dx1, xh1, S["rstd1"], q["g1"])
    want_vec[6] = dpre1.sum(0)
    terms.update({4: dx1 * xh1, 5: dx1, 6: dpre1})
    rowtol = lambda ref: wrow * np.abs(ref).max(-1) + vd.TINY
    back = {"dres": (host(dres), dpre1), "dctx": (host(dctx), dpre1 @ q["Wo"]), "G0": (host(G[0]), dpre1)}
    if nstages == 3:
        back.update({"G1": (host(G[1]), dhid), "G2": (host(G[2]), dpre2)})
    for key, (got, ref) in back.items():
        assert np.isfinite(got).all(), key
        worst[key] = ratio(np.abs(got - ref).max(-1), rowtol(ref))
    for i, ref in want_vec.items():
        got = host(vec[i])
        assert np.isfinite(got).all(), i
        worst["vec%d" % i] = ratio(np.abs(got - ref), (wrow[:, None] * np.abs(terms[i])).sum(0) + vd.TINY)
    print("rowchain nstages=%d: worst error / bar %s" % (nstages, {kk: round(v, 3) for kk, v in worst.items()}))
    assert all(v <= 1 for v in worst.values()), {kk: v for kk, v in worst.items() if not v <= 1}


# =================================================================================================================================
# 3. softmax, attention
# =================================================================================================================================
@pytest.mark.parametrize("rows,cols", [(7, 3), (33, 49), (5, 1050)])
def test_softmax_rows_value_domain(cuda, rows, cols):
    """softmax_rows_fwd / bwd: all-equal logits (uniform to one rounding of 1 / cols), one logit 1e4 above the rest (exactly 1.0 and
    0), logits x scale over +-1e4, an ordinary row between them.  Bar: 2e-5 absolute on p (max|ref| = 1) plus 4 u max|z| max p (1 - p)
    for the fp32 rounding of z = s x scale (_value_domain.softmax_tol; 1e-4 on the spread row of 1050 columns, whose two leading
    logits are 1.4 apart at |z| ~ 1e4 - the fp32 NumPy restatement measures the same 9.8e-5); backward 1e-4 max|ref| from the p the
    backward kernel was given.
    measured on MI355X, 2026-10-21 (error / bar): forward 0.001 at (7,3) and (33,49), 0.36 at (5,1050) - the spread row; backward 0.001."""
    from boosted_detr_amd import kernels as k
    s, names = vd.softmax_input(rows, cols, seed=50)
    scale = vd.SOFTMAX_SCALE
    pt = k.softmax_rows_fwd(dev(s), scale)
    p = host(pt)
    ref = vd.softmax64(s, scale)
    assert np.isfinite(p).all()
    wf = ratio(np.abs(p - ref).max(-1), vd.softmax_tol(s, scale, ref))
    for i, n in enumerate(names):
        if n == "equal":
            assert np.abs(p[i] * cols - 1).max() <= 2 * U, (i, np.abs(p[i] * cols - 1).max() / U)
        if n == "onehot":
            assert p[i].max() == 1.0 and np.sort(p[i])[-2] == 0.0 and p[i].argmax() == (3 * i) % cols
    dp = np.random.default_rng(51).standard_normal((rows, cols)).astype(np.float32)
    ds = host(k.softmax_rows_bwd(pt, dev(dp), scale))
    rds = np.float64(np.float32(scale)) * p * (dp - (p * dp).sum(-1, keepdims=True))
    wb = ratio(np.abs(ds - rds).max(), vd.BWD_BAR * np.abs(rds).max())
    print("softmax (%d,%d): forward error / bar = %.4f, backward error / (1e-4 max|ref|) = %.4f" % (rows, cols, wf, wb))
    assert wf <= 1 and wb <= 1


_ATTN_REF = {}


def attn_case(shape, smax, place):
    key = (shape, smax, place)
    if key not in _ATTN_REF:
        B, h, nq, nk = shape
        Q, K, V, dO, scale = vd.attention_input(B, h, nq, nk, smax, place, seed=60)
        _ATTN_REF[key] = (Q, K, V, dO, scale, vd.attention64(Q, K, V, dO, h, scale))
    return _ATTN_REF[key]


@pytest.mark.parametrize("policy", ["mixed", "split", "bf16x3", "fp32"])
@pytest.mark.parametrize("shape", vd.ATTN_SHAPES)
def test_attention_value_domain(cuda, shape, policy):
    """attention_fwd / bwd with Smax = max |q.k| scale in {1, 20, 80} and the dominant key at a random index, in the LAST chunk (the
    running maximum jumps late, alpha collapses) and in the FIRST (every later p flushes towards 0).  Bars: o - the policy's forward
    bar x max(1, Smax) x max|ref|; lse - forward bar x (1 + max|lse|); dq, dk, dv - the policy's backward bar x max(1, Smax) x
    max|ref| (a GEMM's relative error eps becomes eps x Smax absolute on a score, and that much relative on p).
    measured on MI355X, 2026-10-21 (worst error / bar over the three shapes): o 0.053 (mixed, fp32), 0.038 (split), 0.127 (bf16x3); lse
    0.026 / 0.020 / 0.098; dq 0.037, dk 0.065, dv 0.034 under the 16-bit gradient products, 0.011 / 0.007 / 0.005 under fp32."""
    from boosted_detr_amd import kernels as k
    B, h, nq, nk = shape
    fwd, bwd = vd.ATTN_FWD[policy], vd.ATTN_BWD[policy]
    worst = {}
    for smax in vd.ATTN_SMAX:
        for place in vd.ATTN_PLACEMENTS:
            Q, K, V, dO, scale, ref = attn_case(shape, smax, place)
            with k.gemm_precision(policy):
                o, lse = k.attention_fwd(dev(Q), dev(K), dev(V), h, scale)
                dq, dk, dv = k.attention_bwd(dev(Q), dev(K), dev(V), o, dev(dO), lse, h, scale)
            got = {"o": host(o), "lse": host(lse), "dq": host(dq), "dk": host(dk), "dv": host(dv)}
            amp = max(1.0, smax)
            tol = {"o": fwd * amp * np.abs(ref["o"]).max(), "lse": fwd * (1 + np.abs(ref["lse"]).max())}
            tol.update({n: bwd * amp * np.abs(ref[n]).max() for n in ("dq", "dk", "dv")})
            for n in tol:
                assert got[n].shape == ref[n].shape
                q = ratio(np.abs(got[n] - ref[n]).max(), tol[n])
                worst[n] = max(worst.get(n, 0.0), q)
                assert q <= 1, (policy, shape, smax, place, n, q)
    print("attention %s %s: worst error / bar %s" % (policy, shape, {n: round(v, 4) for n, v in worst.items()}))


# =================================================================================================================================
# 4. pointwise
# =================================================================================================================================
def test_pointwise_saturation_and_specials(cuda):
    """sigmoid / boxsigmoid forward and backward, tanh_bwd, relu_bwd on 1027 values: +-{0, 1e-30, 1e-8, 1, 20, 87, 89, 104, 1e4, 3e38,
    inf}, -0.0 and NaN.  sigmoid and boxsigmoid (= 3 sigmoid(x / 100) - 1): within 2u of fp64, absolute.  Saturated units give
    gradient exactly 0, NaN gives NaN, no finite input gives NaN (exp(x) / (1 + exp(x)) would at 89).
    measured on MI355X, 2026-10-21: sigmoid 0.32 u, boxsigmoid 1.51 u."""
    from boosted_detr_amd import kernels as k
    x = vd.pointwise_input()
    nan = np.isnan(x)
    fin = ~nan
    xd = dev(x)
    dy = np.random.default_rng(70).standard_normal(x.size).astype(np.float32) + np.float32(2.0)
    y = k.sigmoid_fwd(xd)
    yh = host(y)
    assert np.isnan(yh[nan]).all() and not np.isnan(yh[fin]).any()
    e1 = np.abs(yh[fin] - vd.sigmoid64(x[fin])).max()
    assert e1 <= 2 * U, e1 / U
    assert (yh[x >= np.float32(20)] > 0.999).all() and (yh[x >= np.float32(87)] == 1.0).all() and (yh[x <= np.float32(-104)] == 0.0).all()
    g = host(k.sigmoid_bwd(y, dev(dy)))
    ref_g = dy.astype(np.float64) * yh * (1 - yh)
    assert np.isnan(g[nan]).all() and np.abs(g[fin] - ref_g[fin]).max() <= vd.BWD_BAR * np.abs(ref_g[fin]).max()
    assert (g[fin & ((yh == 1.0) | (yh == 0.0))] == 0.0).all()
    b = k.boxsigmoid_fwd(xd)
    bh = host(b)
    ref_b = 3 * vd.sigmoid64((x[fin] / np.float32(100)).astype(np.float32)) - 1
    assert np.isnan(bh[nan]).all() and not np.isnan(bh[fin]).any()
    e2 = np.abs(bh[fin] - ref_b).max()
    assert e2 <= 2 * U, e2 / U
    assert (bh[x >= np.float32(1e4)] == 2.0).all() and (bh[x <= np.float32(-1e4)] == -1.0).all()
    gb = host(k.boxsigmoid_bwd(b, dev(dy)))
    sb = (bh + 1) / 3
    ref_gb = dy.astype(np.float64) * 3 * sb * (1 - sb) / 100
    assert np.isnan(gb[nan]).all() and np.abs(gb[fin] - ref_gb[fin]).max() <= vd.BWD_BAR * np.abs(ref_gb[fin]).max()
    assert (gb[fin & ((bh == 2.0) | (bh == -1.0))] == 0.0).all()
    # tanh_bwd / relu_bwd take the forward OUTPUT: tanh of the values (saturating at +-1), and the values themselves for ReLU
    with np.errstate(invalid="ignore"):
        t = np.tanh(x.astype(np.float64)).astype(np.float32)
    gt = host(k.tanh_bwd(dev(t), dev(dy)))
    ref_t = dy.astype(np.float64) * (1 - t.astype(np.float64) ** 2)
    assert np.isnan(gt[nan]).all() and np.abs(gt[fin] - ref_t[fin]).max() <= 2 * U * np.abs(dy).max()
    assert (gt[fin & (np.abs(t) == 1.0)] == 0.0).all() and (np.abs(t[np.abs(x) >= 20]) == 1.0).all()
    gr = host(k.relu_bwd(xd, dev(dy)))
    assert np.array_equal(gr[fin], np.where(x[fin] > 0, dy[fin], np.float32(0)).astype(np.float64))
    assert (gr[nan] == 0).all()                    # NaN > 0 is false: the unit passes no gradient
    assert (gr[(x == 0)] == 0).all()               # +0.0 and -0.0
    print("pointwise: sigmoid %.2f u (bar 2u), boxsigmoid %.2f u (bar 2u)" % (e1 / U, e2 / U))


# =================================================================================================================================
# 5. optimiser norms and clipping
# =================================================================================================================================
def opt_variables(ws):
    from boosted_detr_amd.engine import Variable, to_device
    vs = []
    for i, w in enumerate(ws):
        v = Variable("vd/t%d/kernel" % i, (w.size,))
        v.value = to_device(w)
        vs.append(v)
    return vs


def load_grads(opt, gs):
    for gv, g in zip(opt.grad_views, gs):
        gv.copy_(torch.from_numpy(g).to(gv.device).view(gv.shape))


def flat(t):
    return t.detach().cpu().contiguous().numpy().ravel().copy()


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_optimiser_norms_and_clipping_over_forty_decades(cuda, kind):
    """bdetr_sgd_nesterov_clipnorm / bdetr_adamw_clipnorm on tensors of 5, 16384 + 3 and 40000 elements; over three steps each tensor
    sees gradients of scale 1e-25 (squares underflow: norm 0, no clipping - the true norm is below clipnorm anyway), 1 and 1e15
    (squares and slab sums finite, clipping active).  The update must equal the fp64 restatement to the bars of the older tests:
    SGD 2e-6 max|w| + 1e-7 (test_training_gpu.py), AdamW 4 x the fp32 restatement's error + 1 ulp (test_adamw_gpu.py).
    measured on MI355X, 2026-10-21 (worst error / bar): SGD 0.026, AdamW 0.220."""
    from boosted_detr_amd.training import SGD, AdamW
    lr, wd = (0.05, 0.0) if kind == "sgd" else (1e-3, 1e-2)
    ws, _ = vd.opt_tensors(vd.OPT_SCALES, seed=80)
    vs = opt_variables(ws)
    opt = SGD(learning_rate=lr, momentum=0.9, nesterov=True, clipnorm=R.CLIPNORM) if kind == "sgd" else AdamW(lr, weight_decay=wd, clipnorm=R.CLIPNORM)
    opt.build(vs)
    w = [x.copy() for x in ws]
    slots = [[np.zeros_like(x) for x in ws] for _ in range(2)]
    worst = 0.0
    for step in range(3):
        scales = [vd.OPT_SCALES[(i + step) % 3] for i in range(3)]
        _, gs = vd.opt_tensors(scales, seed=81 + step)
        load_grads(opt, gs)
        opt.apply_gradients()
        torch.cuda.synchronize()
        for i, var in enumerate(vs):
            got_w = flat(var.value)
            assert np.isfinite(got_w).all(), (kind, step, i, scales[i])
            if kind == "sgd":
                w_ref, v_ref = R.sgd_step64(w[i], gs[i], slots[0][i], lr=lr, clipnorm=R.CLIPNORM)
                got_v = flat(opt.mom_views[i])
                for got, ref in ((got_w, w_ref), (got_v, v_ref)):
                    tol = 2e-6 * np.abs(ref).max() + 1e-7
                    worst = max(worst, ratio(np.abs(got - ref).max(), tol))
                w[i], slots[0][i] = got_w, got_v
            else:
                kw = dict(lr=lr, wd=wd, t=step + 1, clipnorm=R.CLIPNORM, decay=True)
                ref64 = R.adamw_step64(w[i], gs[i], slots[0][i], slots[1][i], **kw)
                ref32 = R.adamw_step32(w[i], gs[i], slots[0][i], slots[1][i], **kw)
                got = (got_w, flat(opt.m_views[i]), flat(opt.v_views[i]))
                for q, a, b_, c in zip("wmv", got, ref64, ref32):
                    err_k, err_r = np.abs(a.astype(np.float64) - b_).max(), np.abs(c.astype(np.float64) - b_).max()
                    floor = float(np.spacing(np.float32(np.abs(b_).max())))
                    worst = max(worst, ratio(err_k, 4 * err_r + floor))
                w[i], slots[0][i], slots[1][i] = got
            clipped = float(np.linalg.norm(gs[i].astype(np.float64))) > R.CLIPNORM
            assert clipped == (scales[i] != 1e-25)
    print("%s over scales 1e-25 / 1 / 1e15: worst error / bar %.3f" % (kind, worst))
    assert worst <= 1


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_optimiser_overflowing_norm_raises_the_guard_and_applies_nothing(cuda, kind):
    """Gradients of scale 1e19: finite, but their squares' slab sums overflow - the norm pass must raise the guard and the apply pass
    leave w and the slots bit-unchanged (every tensor, also the 5-element one)."""
    from boosted_detr_amd import kernels as K
    from boosted_detr_amd.training import SGD, AdamW
    ws, _ = vd.opt_tensors(vd.OPT_SCALES, seed=80)
    vs = opt_variables(ws)
    opt = SGD(learning_rate=0.05, momentum=0.9, nesterov=True, clipnorm=R.CLIPNORM) if kind == "sgd" else AdamW(1e-3, weight_decay=1e-2, clipnorm=R.CLIPNORM)
    opt.build(vs)
    slot_views = (lambda: list(opt.mom_views)) if kind == "sgd" else (lambda: list(opt.m_views) + list(opt.v_views))
    _, gs = vd.opt_tensors([1.0, 1.0, 1.0], seed=90)
    load_grads(opt, gs)
    opt.apply_gradients()                                   # one applied step: non-zero slots
    torch.cuda.synchronize()
    before = [v.value.clone() for v in vs] + [t.clone() for t in slot_views()]
    _, big = vd.opt_tensors([vd.OPT_OVERFLOW] * 3, seed=91)
    assert all(np.isfinite(g).all() for g in big)
    load_grads(opt, big)
    flag = K.overflow_flag()
    flag.zero_()
    try:
        opt.apply_gradients(skip_flag=flag)
        torch.cuda.synchronize()
        assert int(flag.item()) == 1, "the guard did not rise"
        after = [v.value for v in vs] + slot_views()
        assert all(torch.equal(a, b) for a, b in zip(before, after)), "weights or slots touched while the guard is up"
        assert K.read_and_clear_overflow() is True
    finally:
        flag.zero_()
