"""Value-domain inputs and error models for tests/test_value_domain_cpu.py and tests/test_value_domain_gpu.py (NumPy / torch-CPU only).

The other kernel tests draw `randn * small + small`; on such data a one-pass E[x^2] - m^2 LayerNorm, a softmax without the max
subtraction or a variance that goes slightly negative look like a right kernel.  The generators here give every channel / row its own
REGIME (r = |mean| / sigma up to 1000, sigma down to 1e-3, constant, 1e-20, 1e15, 1e19), and the bars are error models in
u = 2^-24 - never constants tuned to what a kernel gives.  Every reference is fp64, computed from the fp32-rounded inputs.

Notation: u = 2^-24; r = |mean| / sigma of a channel or row; R = the number of fp32 additions on the longest chain of a producer
of BatchNorm partial sums; "project bar" = the tolerance the older test of the same kernel uses (2e-5 x max|ref| forward, 1e-4
backward; DESIGN.md's per-policy attention bars)."""
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126           # smallest normal fp32: the absolute floor of a quantity whose terms may flush or lose bits below it
FWD_BAR, BWD_BAR = 2e-5, 1e-4

# ---------------------------------------------------------------------------------------------------------------------------------
# 1. BatchNorm
# ---------------------------------------------------------------------------------------------------------------------------------
# (name, r, sigma).  "const": sigma = 0 at the successive values of BN_CONSTANTS; "tiny": 1e-20 * randn (squares underflow).
BN_REGIMES = [("r0_s1", 0.0, 1.0), ("r1000_s1", 1000.0, 1.0), ("const", None, 0.0), ("tiny", 0.0, 1e-20), ("r10_s1e-3", 10.0, 1e-3),
              ("r100_s1", 100.0, 1.0), ("r1000_s1e-3", 1000.0, 1e-3), ("r100_s1e-3", 100.0, 1e-3), ("r10_s1", 10.0, 1.0),
              ("r0_s1e-3", 0.0, 1e-3)]
# squares of the first three are not representable: the raw E[x^2] - m^2 of fp32 moments goes negative for some of them.  The
# dyadic ones (and 0) have exact fp32 sums at every row count used here: mean == x bit for bit, out == beta exactly.
BN_CONSTANTS = [1000.1, 3.3, -77.7, 0.5, -1024.0, 0.0]
BN_DYADIC = {0.5, -1024.0, 0.0}
BN_HUGE = 1e19              # squares overflow fp32: the statistics are not finite, the range guard must rise


def bn_regime_names(C, start=0, rmax=None):
    """Regime name of every channel: channel c takes BN_REGIMES[(start + c) % 10]; with rmax, regimes of larger r fall back to r0_s1."""
    out = []
    for c in range(C):
        name, r, _ = BN_REGIMES[(start + c) % len(BN_REGIMES)]
        if rmax is not None and r is not None and r > rmax:
            name = "r0_s1"
        out.append(name)
    return out


def bn_targets(C, start=0, rmax=None):
    """(names, mean[C], sigma[C]) float64 nominal values per channel."""
    names = bn_regime_names(C, start, rmax)
    table = {n: (r, s) for n, r, s in BN_REGIMES}
    mean, sigma, k = np.zeros(C), np.zeros(C), 0
    consts = [v for v in BN_CONSTANTS if rmax is None or abs(v) <= rmax]          # (with rmax: the offsets stay below it too)
    for c, n in enumerate(names):
        r, s = table[n]
        if n == "const":
            mean[c], sigma[c] = consts[k % len(consts)], 0.0
            k += 1
        else:
            mean[c], sigma[c] = r * s * (-1.0 if c % 4 == 3 else 1.0), s
    return names, mean, sigma


def bn_input(rows, C, seed=0, start=0, rmax=None):
    """x [rows, C] float32 whose channel c follows its regime, and the regime names."""
    names, mean, sigma = bn_targets(C, start, rmax)
    z = np.random.default_rng(seed).standard_normal((rows, C))
    return (mean[None, :] + sigma[None, :] * z).astype(np.float32), names


def moments64(x):
    """fp64 two-pass (mean, biased variance) over axis 0 of the fp32 data the kernel received."""
    x = np.asarray(x, np.float64)
    m = x.mean(0)
    return m, ((x - m) ** 2).mean(0)


def bn_bounds(m, var, R):
    """The error law of fp32 moment partials with fp64 fold and finalisation: (|dmean|, |dvar|) bounds per channel."""
    m, var = np.abs(np.asarray(m, np.float64)), np.asarray(var, np.float64)
    s = np.sqrt(var)
    return (R + 2) * U * (m + s) + TINY, (R + 2) * U * (m * m + var) + TINY


def rstd_bound(var, eps, dvar):
    rstd = 1.0 / np.sqrt(np.asarray(var, np.float64) + eps)
    return 0.5 * rstd ** 3 * dvar + 2 * U * rstd


def moment_model(x, rows_per_partial, fold32=None):
    """NumPy model of the kernels' scheme: fp32 partial sums of x and x*x over `rows_per_partial` rows each (sequential fp32
    additions), optionally a second fp32 level that folds the partials to `fold32` rows as fold_partials2_kernel does (output row o
    sums partials o, o + fold32, ...), then an fp64 fold and E[x^2] - m^2 in fp64.  Returns (mean, RAW variance - not clamped)."""
    x = np.asarray(x, np.float32)
    rows, C = x.shape
    nparts = -(-rows // rows_per_partial)
    xp = np.zeros((nparts * rows_per_partial, C), np.float32)
    xp[:rows] = x
    xp = xp.reshape(nparts, rows_per_partial, C)
    s, q = np.zeros((nparts, C), np.float32), np.zeros((nparts, C), np.float32)
    for i in range(rows_per_partial):
        v = xp[:, i, :]
        s = (s + v).astype(np.float32)
        q = (q + (v * v).astype(np.float32)).astype(np.float32)
    if fold32:
        fs, fq = np.zeros((fold32, C), np.float32), np.zeros((fold32, C), np.float32)
        for p in range(nparts):
            fs[p % fold32] = fs[p % fold32] + s[p]
            fq[p % fold32] = fq[p % fold32] + q[p]
        s, q = fs, fq
    m = s.astype(np.float64).sum(0) / rows
    return m, q.astype(np.float64).sum(0) / rows - m * m


def bn_apply_tol(ref, mean, var, gamma, eps, bar=FWD_BAR):
    """Per-channel bar of the apply / backward checks against fp64 WITH THE KERNEL'S OWN mean and rstd: the project bar on the
    tensor's magnitude plus 8 u r |gamma| for the one rounding of mean and of x - mean relative to sigma.  For a channel of sigma
    below sqrt(eps) the yardstick is sqrt(var + eps), which is what the kernel divides by (a constant channel has r = inf)."""
    r = np.abs(mean) / np.sqrt(np.asarray(var, np.float64) + eps)
    return bar * np.abs(ref).max(0) + 8 * U * r * np.abs(gamma) * (bar / FWD_BAR) + TINY


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------------
# (name, mean, sigma).  "const" 3.3: not dyadic, the fp32 row sum rounds; "const2" -4.0: every fp32 partial sum is exact.
LN_REGIMES = [("r0", 0.0, 1.0), ("r10", 10.0, 1.0), ("r100", -100.0, 1.0), ("r1000", 1000.0, 1.0), ("const", 3.3, 0.0),
              ("const2", -4.0, 0.0), ("tiny", 0.0, 1e-20), ("big", 0.0, 1e15)]


def ln_regime_names(rows, start=0):
    return [LN_REGIMES[(start + i) % len(LN_REGIMES)][0] for i in range(rows)]


def ln_input(rows, D, seed=0, start=0):
    """[rows, D] float32, row i in regime LN_REGIMES[(start + i) % 8]; and the names."""
    z = np.random.default_rng(seed).standard_normal((rows, D))
    x = np.empty((rows, D))
    for i in range(rows):
        _, m, s = LN_REGIMES[(start + i) % len(LN_REGIMES)]
        x[i] = m + s * z[i]
    return x.astype(np.float32), ln_regime_names(rows, start)


def ln_ref64(h, gamma, beta, eps):
    """fp64 LayerNorm of h [rows, D]: (out, mean, rstd, xhat)."""
    h = np.asarray(h, np.float64)
    m = h.mean(-1, keepdims=True)
    var = ((h - m) ** 2).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xh = (h - m) * rstd
    return xh * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64), m[:, 0], rstd[:, 0], xh


def ln_r(h, eps):
    """r per row with sqrt(var + eps) as the yardstick (equal to |mean| / sigma wherever sigma^2 >> eps; finite for a constant row)."""
    h = np.asarray(h, np.float64)
    return np.abs(h.mean(-1)) / np.sqrt(h.var(-1) + eps)


def ln_fwd_tol(ref, h, gamma, eps, bar=FWD_BAR):
    """Per-row bar [rows]: project bar x max|ref| + (2 + log2 D) u r max|gamma| (the rounding of x + y, of the fp32 mean over a
    log2 D deep tree and of h - mean, relative to sigma)."""
    D = np.asarray(h).shape[-1]
    return bar * np.abs(ref).max() + (2 + math.log2(D)) * U * ln_r(h, eps) * np.abs(gamma).max()


def ln_bwd_factor(h, gamma, eps):
    """Per-row relative widening of the 1e-4 backward bar: (2 + log2 D) u r max|gamma|."""
    D = np.asarray(h).shape[-1]
    return (2 + math.log2(D)) * U * ln_r(h, eps) * np.abs(gamma).max()


def ln_two_pass32(h, gamma, beta, eps):
    """fp32 NumPy two-pass restatement (what the kernels do, up to the order of additions)."""
    f = np.float32
    h = np.asarray(h, f)
    D = h.shape[-1]
    m = (h.sum(-1, dtype=f) / f(D)).astype(f)[:, None]
    t = (h - m).astype(f)
    var = ((t * t).sum(-1, dtype=f) / f(D)).astype(f)[:, None]
    rstd = (f(1) / np.sqrt(var + f(eps))).astype(f)
    return ((t * rstd) * np.asarray(gamma, f) + np.asarray(beta, f)).astype(f), rstd[:, 0]


def ln_one_pass32(h, gamma, beta, eps):
    """The WRONG kind: fp32 sum(h^2) / D - mean^2 (no clamp).  Random inputs cannot tell it from ln_two_pass32; r = 1000 can."""
    f = np.float32
    h = np.asarray(h, f)
    D = h.shape[-1]
    m = (h.sum(-1, dtype=f) / f(D)).astype(f)[:, None]
    var = ((h * h).sum(-1, dtype=f) / f(D) - (m * m)[:, 0]).astype(f)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        rstd = (f(1) / np.sqrt(var + f(eps))).astype(f)
        return (((h - m) * rstd) * np.asarray(gamma, f) + np.asarray(beta, f)).astype(f), rstd[:, 0]


def ln_bwd64(dout, xh, rstd, gamma):
    """fp64 LayerNorm input gradient and (dgamma, dbeta)."""
    g = dout * gamma
    dh = (g - g.mean(-1, keepdims=True) - xh * (g * xh).mean(-1, keepdims=True)) * rstd[:, None]
    return dh, (dout * xh).sum(0), dout.sum(0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. softmax and attention
# ---------------------------------------------------------------------------------------------------------------------------------
SOFTMAX_REGIMES = ["equal", "onehot", "spread", "ordinary"]
SOFTMAX_SCALE = 0.17677669


def softmax_input(rows, cols, seed=0, scale=SOFTMAX_SCALE):
    """Logits [rows, cols] float32 (the kernel multiplies by `scale`): all-equal, one entry 1e4 (after the scale) above the rest,
    logits x scale spread over +-1e4, and an ordinary randn * 3 row between them; names."""
    rng = np.random.default_rng(seed)
    s = np.empty((rows, cols))
    names = []
    for i in range(rows):
        kind = SOFTMAX_REGIMES[i % 4]
        names.append(kind)
        if kind == "equal":
            s[i] = [7.25, -3.0e3, 0.0][(i // 4) % 3]
        elif kind == "onehot":
            s[i] = rng.standard_normal(cols)
            s[i, (3 * i) % cols] += 1e4 / scale
        elif kind == "spread":
            s[i] = rng.uniform(-1e4, 1e4, cols) / scale
        else:
            s[i] = rng.standard_normal(cols) * 3
    return s.astype(np.float32), names


def softmax64(s, scale):
    z = np.asarray(s, np.float64) * np.float64(np.float32(scale))
    z = z - z.max(-1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(-1, keepdims=True)


def softmax_tol(s, scale, ref, bar=FWD_BAR):
    """Per-row bar on p [rows]: the project bar (absolute, max|ref| <= 1) plus 4 u max|z| max p (1 - p), z = s x scale.  The kernel
    forms z in fp32: u |z| absolute on a score and on the row maximum, 2 u max|z| on z - max, that much RELATIVE on exp, and twice
    that times p (1 - p) on p after the normalisation - the law the attention bars follow with Smax.  It vanishes for one-hot
    rows; at |z| = 1e4 with two leading logits a few units apart it is 1e-4, which the fp32 restatement shows as well."""
    z = np.abs(np.asarray(s, np.float64) * scale).max(-1)
    return bar + 4 * U * z * (ref * (1 - ref)).max(-1)


def softmax32(s, scale, subtract_max=True):
    f = np.float32
    z = (np.asarray(s, f) * f(scale)).astype(f)
    if subtract_max:
        z = (z - z.max(-1, keepdims=True)).astype(f)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(z).astype(f)
        return (e / e.sum(-1, keepdims=True, dtype=f)).astype(f)


ATTN_SHAPES = [(1, 4, 50, 49), (1, 8, 33, 65), (1, 4, 70, 130)]       # one ragged chunk; a second chunk of ONE key; three chunks, two workgroup columns
ATTN_SMAX = [1.0, 20.0, 80.0]
ATTN_PLACEMENTS = ["random", "last", "first"]
ATTN_CHUNK = 64             # keys per chunk of the online softmax (csrc/attention.hip)
ATTN_FWD = {"mixed": 1e-5, "split": 1e-5, "fp32": 1e-5, "bf16x3": 5e-5}
ATTN_BWD = {"mixed": 2e-4, "split": 2e-4, "fp32": 1e-4, "bf16x3": 2e-4}


def attention_input(B, h, nq, nk, smax, placement, seed=0, d=32):
    """(Q [B,nq,h*d], K, V [B,nk,h*d], dO [B,h,nq,d], scale) float32.  Every (batch, head) has ONE dominant key - each query is
    0.3 randn + the key's direction - at a random index, in the last chunk (the running maximum jumps late, alpha collapses) or in
    the first (every later p flushes towards 0).  Q is then scaled so that max |q . k| * scale == smax."""
    rng = np.random.default_rng(seed)
    scale = 1.0 / math.sqrt(d)
    Q = 0.3 * rng.standard_normal((B, h, nq, d))
    K = rng.standard_normal((B, h, nk, d))
    V = rng.standard_normal((B, h, nk, d))
    dO = rng.standard_normal((B, h, nq, d))
    last0 = (nk - 1) // ATTN_CHUNK * ATTN_CHUNK
    for b in range(B):
        for j in range(h):
            if placement == "random":
                idx = int(rng.integers(nk))
            elif placement == "last":
                idx = last0 + int(rng.integers(nk - last0))
            else:
                idx = int(rng.integers(min(ATTN_CHUNK, nk)))
            Q[b, j] += K[b, j, idx] / np.linalg.norm(K[b, j, idx])
    Q *= smax / (np.abs(Q @ K.transpose(0, 1, 3, 2)).max() * scale)
    pack = lambda t: np.ascontiguousarray(t.transpose(0, 2, 1, 3)).reshape(B, t.shape[2], h * d).astype(np.float32)
    return pack(Q), pack(K), pack(V), dO.astype(np.float32), scale


def heads(t, h, d=32):
    """[B, n, h*d] -> [B, h, n, d] float64"""
    B, n, _ = t.shape
    return np.asarray(t, np.float64).reshape(B, n, h, d).transpose(0, 2, 1, 3)


def attention64(Q, K, V, dO, h, scale):
    """fp64 reference from the fp32 inputs: dict o [B,h,nq,d], lse [B,h,nq], dq/dk/dv in the packed [B,n,h*d] layout, smax."""
    q, k, v, do = heads(Q, h), heads(K, h), heads(V, h), np.asarray(dO, np.float64)
    s = q @ k.transpose(0, 1, 3, 2) * scale
    mx = s.max(-1, keepdims=True)
    e = np.exp(s - mx)
    l = e.sum(-1, keepdims=True)
    p = e / l
    o = p @ v
    dv = p.transpose(0, 1, 3, 2) @ do
    dp = do @ v.transpose(0, 1, 3, 2)
    ds = p * (dp - (dp * p).sum(-1, keepdims=True)) * scale
    unpack = lambda t: t.transpose(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], -1)
    return {"o": o, "lse": (mx + np.log(l))[..., 0], "dq": unpack(ds @ k), "dk": unpack(ds.transpose(0, 1, 3, 2) @ q), "dv": unpack(dv),
            "smax": float(np.abs(s).max())}


def attention_online32(Q, K, V, h, scale):
    """fp32 NumPy restatement of the online softmax in the log2 domain, ATTN_CHUNK keys at a time: (o, lse)."""
    f = np.float32
    q, k, v = (heads(t, h).astype(f) for t in (Q, K, V))
    nk = k.shape[2]
    c = f(scale * math.log2(math.e))
    m = np.full(q.shape[:3] + (1,), -np.inf, f)
    l = np.zeros_like(m)
    o = np.zeros(q.shape, f)
    for j0 in range(0, nk, ATTN_CHUNK):
        s = ((q @ k[:, :, j0:j0 + ATTN_CHUNK].transpose(0, 1, 3, 2)).astype(f) * c).astype(f)
        mn = np.maximum(m, s.max(-1, keepdims=True))
        alpha = np.exp2(m - mn).astype(f)
        p = np.exp2(s - mn).astype(f)
        l = (l * alpha + p.sum(-1, keepdims=True, dtype=f)).astype(f)
        o = (o * alpha + (p @ v[:, :, j0:j0 + ATTN_CHUNK]).astype(f)).astype(f)
        m = mn
    return (o / l).astype(f), ((m + np.log2(l).astype(f)) * f(math.log(2.0))).astype(f)[..., 0]


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. pointwise
# ---------------------------------------------------------------------------------------------------------------------------------
POINTWISE_MAGNITUDES = [0.0, 1e-30, 1e-8, 1.0, 20.0, 87.0, 89.0, 104.0, 1e4, 3e38, np.inf]
POINTWISE_N = 1027           # 256 quads and a 3-element tail


def pointwise_input():
    """1027 float32 values: +-POINTWISE_MAGNITUDES (so +0.0 and -0.0 both) and NaN, repeated to the length: every value sits in
    a quad somewhere and the last three in the tail."""
    base = [s * v for v in POINTWISE_MAGNITUDES for s in (1.0, -1.0)] + [np.nan]
    reps = -(-POINTWISE_N // len(base))
    return np.asarray((base * reps)[:POINTWISE_N], np.float32)


def sigmoid64(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


def sigmoid32(x, naive=False):
    f = np.float32
    x = np.asarray(x, f)
    with np.errstate(over="ignore", invalid="ignore"):
        if naive:
            e = np.exp(x).astype(f)
            return (e / (f(1) + e)).astype(f)
        return (f(1) / (f(1) + np.exp(-x).astype(f))).astype(f)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. optimiser norms
# ---------------------------------------------------------------------------------------------------------------------------------
OPT_SIZES = [5, 16384 + 3, 40000]
OPT_SCALES = [1e-25, 1.0, 1e15]
OPT_OVERFLOW = 1e19


def opt_tensors(scale_of, seed=0):
    """(weights, gradients) float32 lists for OPT_SIZES; gradient i = scale_of[i] * randn."""
    rng = np.random.default_rng(seed)
    ws = [(0.05 * rng.standard_normal(n)).astype(np.float32) for n in OPT_SIZES]
    gs = [(s * rng.standard_normal(n)).astype(np.float32) for n, s in zip(OPT_SIZES, scale_of)]
    return ws, gs
