"""The generators and bars of tests/_value_domain.py are sound (no GPU): every generator produces every regime it names, the fp32
NumPy restatement of each kernel family meets the bars the GPU tests hold the kernels to - and the restatements that are wrong in
kind (raw negative variance, one-pass LayerNorm, softmax without the max, exp(x) / (1 + exp(x))) miss them, which random inputs
never show."""
import math

import numpy as np
import pytest

import _adamw_ref as R
import _value_domain as vd

U, EPS = vd.U, 1.001e-5


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
@pytest.mark.parametrize("rows,C,start", [(98, 64, 0), (800, 64, 0), (9600, 8, 0), (9600, 8, 5), (130, 48, 0), (28, 64, 0)])
def test_bn_generator_produces_every_regime(rows, C, start):
    x, names = vd.bn_input(rows, C, seed=1, start=start)
    want = {n for n, _, _ in vd.BN_REGIMES}
    seen = set(names) | (set(vd.bn_regime_names(C, 0) + vd.bn_regime_names(C, 5)) if C < 10 else set())      # C = 8 is run at start 0 AND 5
    assert seen == want, want - seen
    m, var = vd.moments64(x)
    table = {n: (r, s) for n, r, s in vd.BN_REGIMES}
    consts = []
    for c, n in enumerate(names):
        r, s = table[n]
        if n == "const":
            assert var[c] == 0 and np.all(x[:, c] == x[0, c])
            consts.append(float(x[0, c]))
        else:
            # sample moments of `rows` draws: sigma within 6 / sqrt(2 rows), mean within 6 sigma / sqrt(rows)
            assert abs(math.sqrt(var[c]) / s - 1) < 6 / math.sqrt(2 * rows), (n, var[c])
            assert abs(abs(m[c]) - r * s) < 6 * s / math.sqrt(rows), (n, m[c])
    if C >= 48:
        assert {np.float32(v) for v in vd.BN_CONSTANTS[:C // 10]} <= {np.float32(v) for v in consts}
    assert np.isfinite(x).all() and x.dtype == np.float32


def test_constant_channels_give_a_negative_raw_variance_in_the_moment_model():
    """What tests the `var < 0` clamp: fp32 sums of x and of the ROUNDED x * x of a constant whose square is not representable leave
    E[x^2] - m^2 below zero for some columns.  (Were it never negative, the GPU test could not see a missing clamp.)"""
    neg = 0
    for rows, C, rpp in [(98, 64, 4), (800, 64, 4), (9600, 8, 32), (130, 48, 2)]:
        for start in (0, 5):
            x, names = vd.bn_input(rows, C, seed=1, start=start)
            _, raw = vd.moment_model(x, rpp)
            cols = [c for c, n in enumerate(names) if n == "const"]
            neg += int((raw[cols] < 0).sum())
            with np.errstate(invalid="ignore"):
                assert np.isnan(1.0 / np.sqrt(raw[cols][raw[cols] < -EPS] + EPS)).all()          # ... and past -eps the square root is NaN
    assert neg >= 1, "no constant column of the generator drives the raw variance negative"
    x, names = vd.bn_input(800, 64, seed=1)
    _, raw = vd.moment_model(x, 4)
    worst = min(raw[c] for c, n in enumerate(names) if n == "const")
    print("most negative raw variance of a constant channel (rows 800, 4-row partials): %.3e (eps %.3e)" % (worst, EPS))
    assert worst < -EPS, "no constant channel takes var + eps below zero: a missing clamp would not give NaN"


@pytest.mark.parametrize("rows,C,rpp,fold", [(98, 64, 8, None), (800, 64, 8, None), (9600, 8, 32, None), (9600, 8, 32, 64), (130, 48, 2, None)])
def test_moment_model_meets_the_statistics_bars(rows, C, rpp, fold):
    """|dmean| <= (R + 2) u (|m| + s), |dvar| <= (R + 2) u (m^2 + s^2) with R = rows per partial (+ the fp32 fold depth), the derived
    rstd bound, 0 < rstd <= (1 + 2u) / sqrt(eps) - for the clamped model, at both regime rotations."""
    worst = 0.0
    for start in (0, 5):
        x, names = vd.bn_input(rows, C, seed=2, start=start)
        m64, v64 = vd.moments64(x)
        m, raw = vd.moment_model(x, rpp, fold)
        var = np.maximum(raw, 0)
        Rr = rpp + (-(-(-(-rows // rpp)) // fold) if fold else 0)
        bm, bv = vd.bn_bounds(m64, v64, Rr)
        assert (np.abs(m - m64) <= bm).all() and (np.abs(var - v64) <= bv).all()
        rstd = 1 / np.sqrt(var + EPS)
        assert (np.abs(rstd - 1 / np.sqrt(v64 + EPS)) <= vd.rstd_bound(v64, EPS, bv)).all()
        assert np.isfinite(rstd).all() and (rstd > 0).all() and (rstd <= (1 + 2 * U) / math.sqrt(EPS)).all()
        tiny = [c for c, n in enumerate(names) if n == "tiny"]
        assert np.allclose(rstd[tiny], 1 / math.sqrt(EPS), rtol=U, atol=0)
        worst = max(worst, float((np.abs(var - v64) / (U * (m64 ** 2 + v64) + vd.TINY)).max()))
    print("moment model rows=%d rpp=%d fold=%s: max |dvar| / (u (m^2 + s^2)) = %.2f (bound %d)" % (rows, rpp, fold, worst, Rr + 2))


def test_huge_channel_overflows_the_squares():
    x = (vd.BN_HUGE * np.random.default_rng(0).standard_normal(98)).astype(np.float32)
    with np.errstate(over="ignore"):
        assert np.isfinite(x).all() and not np.isfinite((x * x).sum(dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("rows,D", [(37, 64), (5, 1024), (33, 256), (19, 29)])
def test_layernorm_generator_and_two_pass_restatement(rows, D):
    eps = 1e-3
    rng = np.random.default_rng(3)
    gamma, beta = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32), (0.1 * rng.standard_normal(D)).astype(np.float32)
    seen, worst = set(), 0.0
    for start in (0, 3):
        h, names = vd.ln_input(rows, D, seed=4, start=start)
        seen |= set(names)
        ref, _, rstd64, _ = vd.ln_ref64(h, gamma, beta, eps)
        tol = vd.ln_fwd_tol(ref, h, gamma, eps)
        got, rstd = vd.ln_two_pass32(h, gamma, beta, eps)
        err = np.abs(got - ref).max(-1)
        assert np.isfinite(got).all() and (err <= tol).all(), list(zip(names, err / tol))
        worst = max(worst, float((err / tol).max()))
        for i, n in enumerate(names):
            if n in ("const", "const2", "tiny"):
                assert abs(rstd[i] * math.sqrt(eps) - 1) <= 2 * U
            if n == "const2":
                assert np.array_equal(got[i], beta)                       # exact sums: out == beta bit for bit
            if n == "r1000":
                # the one-pass variance misses the same bar: its variance error is ~ u m^2 / sqrt(D) (the rounded squares, summed
                # pairwise), i.e. up to several % of sigma^2 at r = 1000
                bad, _ = vd.ln_one_pass32(h[i:i + 1], gamma, beta, eps)
                e1 = np.abs(bad - ref[i]).max()
                assert not e1 <= 2 * tol[i], (e1, tol[i])
    assert seen == {n for n, _, _ in vd.LN_REGIMES}
    print("two-pass fp32 restatement (%d, %d): worst error / bar %.3f" % (rows, D, worst))


# ---------------------------------------------------------------------------------------------------------------- softmax, attention
@pytest.mark.parametrize("rows,cols", [(7, 3), (33, 49), (5, 1050)])
def test_softmax_generator_and_restatement(rows, cols):
    s, names = vd.softmax_input(rows, cols, seed=50)
    assert set(names) == set(vd.SOFTMAX_REGIMES) and np.isfinite(s).all()
    ref = vd.softmax64(s, vd.SOFTMAX_SCALE)
    got = vd.softmax32(s, vd.SOFTMAX_SCALE)
    err = np.abs(got - ref).max(-1)
    assert (err <= vd.softmax_tol(s, vd.SOFTMAX_SCALE, ref)).all()
    if cols == 1050:
        # the spread row of this seed has two leading logits 1.4 apart at |z| ~ 1e4: fp32 rounding of s x scale alone costs 1e-4
        # on p, five project bars - the format, not a kernel; hence the u max|z| p (1 - p) term of softmax_tol
        i = names.index("spread")
        assert err[i] > vd.FWD_BAR and err[i] <= vd.softmax_tol(s, vd.SOFTMAX_SCALE, ref)[i]
        print("spread row: fp32 restatement error %.2e, bar %.2e" % (err[i], vd.softmax_tol(s, vd.SOFTMAX_SCALE, ref)[i]))
    for i, n in enumerate(names):
        if n == "equal":
            assert np.abs(got[i].astype(np.float64) * cols - 1).max() <= 2 * U      # exp(0) = 1, the sum is exact, one rounding of 1 / cols
        if n == "onehot":
            assert got[i].max() == 1.0 and np.sort(got[i])[-2] == 0.0
    bad = vd.softmax32(s, vd.SOFTMAX_SCALE, subtract_max=False)
    assert not np.isfinite(bad).all()                                  # without the max subtraction these rows are NaN


def test_attention_restatement_meets_the_bars_with_room():
    worst_o = worst_l = 0.0
    for (B, h, nq, nk) in vd.ATTN_SHAPES:
        for smax in vd.ATTN_SMAX:
            for place in vd.ATTN_PLACEMENTS:
                Q, K, V, dO, scale = vd.attention_input(B, h, nq, nk, smax, place, seed=6)
                ref = vd.attention64(Q, K, V, dO, h, scale)
                assert abs(ref["smax"] / smax - 1) < 1e-5
                o, lse = vd.attention_online32(Q, K, V, h, scale)
                eo = np.abs(o - ref["o"]).max() / (np.abs(ref["o"]).max() * max(1.0, smax))
                el = np.abs(lse - ref["lse"]).max() / (1 + np.abs(ref["lse"]).max())
                worst_o, worst_l = max(worst_o, eo), max(worst_l, el)
                # the dominant key holds most of every row's mass at smax >= 20
                if smax >= 20:
                    p = np.exp(vd.heads(Q, h) @ vd.heads(K, h).transpose(0, 1, 3, 2) * scale - ref["lse"][..., None])
                    assert np.median(p.max(-1)) > 0.5
    print("online-softmax fp32 restatement: o %.1f u max(1, Smax), lse %.1f u (1 + |lse|)" % (worst_o / U, worst_l / U))
    assert worst_o <= 0.5 * min(vd.ATTN_FWD.values()) and worst_l <= 0.5 * min(vd.ATTN_FWD.values())


def test_attention_placements_land_in_the_named_chunk():
    for (B, h, nq, nk) in vd.ATTN_SHAPES:
        for place in ("last", "first"):
            Q, K, V, dO, scale = vd.attention_input(B, h, nq, nk, 80.0, place, seed=6)
            s = vd.heads(Q, h) @ vd.heads(K, h).transpose(0, 1, 3, 2)
            top = np.array([np.bincount(s[0, j].argmax(-1), minlength=nk).argmax() for j in range(h)])
            last0 = (nk - 1) // vd.ATTN_CHUNK * vd.ATTN_CHUNK
            assert (top >= last0).all() if place == "last" else (top < vd.ATTN_CHUNK).all(), (place, top)


# ---------------------------------------------------------------------------------------------------------------- pointwise
def test_pointwise_inputs_and_sigmoid_restatement():
    x = vd.pointwise_input()
    assert x.size == 1027 and x.size % 4 == 3
    for v in vd.POINTWISE_MAGNITUDES:
        assert (x == np.float32(v)).any() and (x == np.float32(-v)).any()
    assert np.isnan(x).any() and (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any()
    fin = ~np.isnan(x)
    ref = vd.sigmoid64(x[fin])
    got = vd.sigmoid32(x)
    assert np.isnan(got[~fin]).all() and np.abs(got[fin] - ref).max() <= 2 * U
    naive = vd.sigmoid32(x, naive=True)
    assert np.isnan(naive[x == np.float32(89.0)]).all()                 # exp(89) overflows: inf / inf
    box = (np.float32(3) * vd.sigmoid32((x / np.float32(100)).astype(np.float32)) - np.float32(1)).astype(np.float32)
    err = np.abs(box[fin] - (3 * vd.sigmoid64((x[fin] / np.float32(100)).astype(np.float32)) - 1)).max()
    # (NumPy's exp: 2.06 u here; 3 x the sigmoid's 2u + u for the result's own rounding in [1, 2) bounds any faithful fp32 form.  The
    # GPU test holds the kernel to 2u, which its expf meets: 1.51 u measured)
    print("boxsigmoid fp32 restatement: %.2f u" % (err / U))
    assert err <= 3 * 2 * U + U


# ---------------------------------------------------------------------------------------------------------------- optimiser
def test_optimiser_gradient_scales_reach_the_named_paths():
    ws, gs = vd.opt_tensors(vd.OPT_SCALES, seed=7)
    assert [g.size for g in gs] == [5, 16387, 40000]
    for g, s in zip(gs, vd.OPT_SCALES):
        n32, n64 = float(R.norm32(g)), float(np.linalg.norm(g.astype(np.float64)))
        if s == 1e-25:
            assert n32 == 0.0 and 0 < n64 < R.CLIPNORM                  # squares underflow; no clipping either way
        else:
            assert np.isfinite(n32) and abs(n32 / n64 - 1) < 1e-5 and n64 > R.CLIPNORM
    _, big = vd.opt_tensors([vd.OPT_OVERFLOW] * 3, seed=7)
    with np.errstate(over="ignore"):
        assert all(np.isfinite(g).all() for g in big) and not np.isfinite(float(R.norm32(big[2])))
