"""Attention masks on the GPU (include/bdetr.h K32-K34): the fused masked forward and both backward kernels of csrc/attention.hip,
the unfused path, and the transformer layers' keywords, against the fp64 restatement in tests/_attention_mask_ref.py.

Bars are those of test_kernels_gpu.test_fused_attention_fwd_bwd, error relative to max|want|: forward and lse 1e-5 (5e-5 under
'bf16x3'), gradients 5e-5 under 'fp32' and 2e-4 otherwise - the mask adds one exactly rounded fp32 multiply per probability.
Shapes: the kernels' constants are 64-key chunks, 32-row tiles and 128 queries per workgroup (4 waves x 32)."""
import functools
import math

import pytest
import torch

import _guard
from _attention_mask_ref import attention_grads, attention_ref

pytestmark = pytest.mark.gpu

POLICIES = ["mixed", "split", "bf16x3", "fp32"]
SHAPES = [(1, 1, 1, 1),          # minimal
          (2, 2, 33, 65),        # a one-key ragged chunk, a wave with one query, idle waves
          (2, 3, 130, 49),       # two workgroups, nk < 64 and not a multiple of 4
          (2, 2, 100, 200)]      # three full chunks plus a ragged 8
FORMS = ["B11k", "11qk", "B1qk", "1h1k", "Bhqk"]
RULES = ["multiply", "exclude"]
HD = 32


def dev(t):
    return t.contiguous().cuda()


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def fwd_tol(policy):
    return 5e-5 if policy == "bf16x3" else 1e-5


def bwd_tol(policy):
    return 5e-5 if policy == "fp32" else 2e-4


def close(got, want, rtol, what="", allow_abs=0.0):
    """test_kernels_gpu.close (max error against rtol * max|want|); a -inf (the lse of a row with no kept key) must be met exactly.
    allow_abs: twice the UNMASKED kernel's own error on the same operands, where a case's docstring says so (0 everywhere else)."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not torch.isnan(got).any(), f"{what}: NaN"
    inf = torch.isinf(want)
    assert torch.equal(got[inf], want[inf]), f"{what}: infinite entries differ"
    got, want = got[~inf], want[~inf]
    if want.numel() == 0:
        return 0.0
    scale = want.abs().max().item() + 1e-30
    err = (got - want).abs().max().item()
    print(f"{what}: max err {err:.3e} of scale {scale:.3e} = {err / scale:.3e} (bar {rtol:.1e})")
    bar = max(rtol * scale, allow_abs)
    assert err <= bar, f"{what}: max err {err:.3e} > {bar:.3e} (scale {scale:.3e}, twice the unmasked kernel's error {allow_abs:.3e})"
    return err / scale


def max_err(got, want):
    return (got.detach().cpu().double() - want.detach().cpu().double()).abs().max().item()


def mask_shape(form, B, h, nq, nk):
    return {"B11k": (B, 1, 1, nk), "11qk": (1, 1, nq, nk), "B1qk": (B, 1, nq, nk), "1h1k": (1, h, 1, nk), "Bhqk": (B, h, nq, nk)}[form]


def make_mask(rule, shape, seed=7):
    g = torch.Generator().manual_seed(seed)
    if rule == "none":
        return None
    if rule == "exclude":
        return torch.rand(shape, generator=g) < 0.5                      # keeps about half the keys
    m = torch.randn(shape, generator=g) * 1.5                            # negatives and values above 1 ...
    m[torch.rand(shape, generator=g) < 0.3] = 0.0                        # ... and zeros
    return m


@functools.lru_cache(maxsize=None)
def operands(B, h, nq, nk, d=HD):
    Q, K, V = rnd(B, nq, h * d, seed=1), rnd(B, nk, h * d, seed=2), rnd(B, nk, h * d, seed=3)
    Q[0, 0] *= 6.0                                                       # a spiky row: exercises the online-softmax rescale
    return Q, K, V, rnd(B, h, nq, d, seed=4)


@functools.lru_cache(maxsize=None)
def case(B, h, nq, nk, form, rule):
    """Operands, mask and the fp64 reference, computed once and shared by the policies (never modified)."""
    Q, K, V, dO = operands(B, h, nq, nk)
    mask = make_mask(rule, mask_shape(form, B, h, nq, nk))
    return Q, K, V, dO, mask, attention_grads(Q, K, V, h, mask, dO)


def run(Q, K, V, dO, h, mask, policy):
    from boosted_detr_amd import kernels as k
    scale = 1.0 / math.sqrt(Q.shape[-1] // h)
    q, kk, v, do = dev(Q), dev(K), dev(V), dev(dO)
    m = None if mask is None else dev(mask)
    with k.gemm_precision(policy):
        o, lse = k.attention_fwd(q, kk, v, h, scale, mask=m) if m is not None else k.attention_fwd(q, kk, v, h, scale)
        dq, dk, dv = (k.attention_bwd(q, kk, v, o, do, lse, h, scale, mask=m) if m is not None
                      else k.attention_bwd(q, kk, v, o, do, lse, h, scale))
    return o, lse, dq, dk, dv


def check(got, want, policy, what, allow=None):
    for name, g, w, tol in zip(("o", "lse", "dq", "dk", "dv"), got, want, (fwd_tol(policy),) * 2 + (bwd_tol(policy),) * 3):
        close(g, w, tol, f"{what} {name}", (allow or {}).get(name, 0.0))


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,h,nq,nk", SHAPES)
def test_masked_attention_fwd_bwd(cuda, B, h, nq, nk, form, rule, policy):
    """Every broadcast form under both rules and every arithmetic policy against fp64; f32 masks hold zeros, negatives and values
    above 1, bool masks keep about half the keys, one query row is spiky.

    One case needs more than the bar and takes the allowance the bars come with (twice the unmasked kernel's error on the same
    Q, K, V): lse at (1,1,1,1) under the multiply rule.  It is the unmasked lse, here a single 32-term dot product of the spiky query
    (terms of magnitude ~6) that cancels to 0.054, so the products' rounding is large against max|want|.  Measured on an MI355X, the
    masked and the unmasked kernel alike (same bits): 1.417e-06 = 2.6e-05 of max|want| under 'mixed' and 'fp32', 2.866e-05 = 5.3e-04
    under 'bf16x3' ('split' meets the bar)."""
    Q, K, V, dO, mask, want = case(B, h, nq, nk, form, rule)
    allow = None
    if (B, h, nq, nk) == (1, 1, 1, 1) and rule == "multiply":
        unmasked = run(Q, K, V, dO, h, None, policy)[1]
        allow = {"lse": 2 * max_err(unmasked, case(B, h, nq, nk, form, "none")[5][1])}
        print(f"unmasked kernel's lse error {allow['lse'] / 2:.3e}")
    check(run(Q, K, V, dO, h, mask, policy), want, policy, f"{rule} {form}", allow)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,h,nq,nk", SHAPES)
def test_all_pass_mask_is_bit_identical_to_unmasked(cuda, B, h, nq, nk, form, rule, policy):
    """An all-ones f32 mask (p * 1.0f is exact) and an all-True bool mask give o, lse, dq, dk, dv bit-identical to the unmasked
    entry points, and two masked calls are bit-identical to each other.  Conditions, not measurements."""
    Q, K, V, dO = operands(B, h, nq, nk)
    mask = torch.ones(mask_shape(form, B, h, nq, nk), dtype=torch.float32 if rule == "multiply" else torch.bool)
    plain = run(Q, K, V, dO, h, None, policy)
    first, second = run(Q, K, V, dO, h, mask, policy), run(Q, K, V, dO, h, mask, policy)
    for name, p, a, b in zip(("o", "lse", "dq", "dk", "dv"), plain, first, second):
        assert torch.equal(a, p), f"{name}: masked differs from unmasked at {(a != p).sum().item()} element(s)"
        assert torch.equal(a, b), f"{name}: two masked calls differ"


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("rule", RULES)
def test_two_masked_calls_are_bit_identical(cuda, rule, policy):
    B, h, nq, nk = 2, 3, 130, 49
    Q, K, V, dO, mask, _ = case(B, h, nq, nk, "Bhqk", rule)
    for a, b in zip(run(Q, K, V, dO, h, mask, policy), run(Q, K, V, dO, h, mask, policy)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ----------------------------------------------------------------------------------------------- dedicated exclusion cases
def exclusion_case(name, B, h, nq, nk):
    """(mask, rows with no kept key as a [B,h,nq] bool)."""
    full = make_mask("exclude", (B, h, nq, nk), seed=11)
    if name == "empty_rows":                     # every key of some rows excluded, in a full mask
        full[0, 0, 0] = False                    # (the spiky query)
        full[B - 1, h - 1, nq - 1] = False
        full[0, :, nq // 2] = False
        return full, ~full.any(-1)
    if name == "empty_rows_key_only":            # a whole image without a kept key
        m = make_mask("exclude", (B, 1, 1, nk), seed=12)
        m[0] = False
        return m, ~m.any(-1).expand(B, h, nq)
    if name == "first_chunk_excluded":           # keys 0..63 excluded, later ones kept: the running maximum starts at -inf
        full[..., :64] = False
        full[..., 64:] |= make_mask("exclude", (B, h, nq, nk - 64), seed=13)
        full[..., nk - 1] = True
        return full, ~full.any(-1)
    if name == "first_chunk_excluded_key_only":
        m = torch.ones(B, 1, 1, nk, dtype=torch.bool)
        m[..., :64] = False
        return m, ~m.any(-1).expand(B, h, nq)
    if name == "only_ragged_tail_key":           # the only kept key lies in the ragged tail
        m = torch.zeros(B, h, nq, nk, dtype=torch.bool)
        m[..., nk - 1] = True
        return m, ~m.any(-1)
    if name == "only_ragged_tail_key_key_only":
        m = torch.zeros(B, 1, 1, nk, dtype=torch.bool)
        m[..., nk - 1] = True
        return m, ~m.any(-1).expand(B, h, nq)
    raise KeyError(name)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("B,h,nq,nk", [(2, 2, 33, 65), (2, 2, 100, 200)])
@pytest.mark.parametrize("name", ["empty_rows", "empty_rows_key_only", "first_chunk_excluded", "first_chunk_excluded_key_only",
                                  "only_ragged_tail_key", "only_ragged_tail_key_key_only"])
def test_exclusion_edge_cases(cuda, name, B, h, nq, nk, policy):
    """Rows with no kept key give O = 0, lse = -inf (compared by equality) and dq = 0; no NaN anywhere; everything else meets the
    reference at the usual bars.

    Where ONE key is kept for every row (the ragged-tail cases, and the first-chunk cases at nk = 65) every probability is exactly
    1, dS = P (dP - D) is exactly 0 in exact arithmetic and max|want| of dq and dk is 0: the kernel's dP (an MFMA product) and D
    (attn_dvec_kernel's fp32 row dot) round differently, and what is left is an absolute residue.  Those two tensors take the
    allowance the bars come with: twice the unmasked kernel's error on the same Q and the kept K[:, j], V[:, j].
    Measured on an MI355X, absolute residues (gradients of order 1), the masked kernels and the unmasked kernel on the kept key
    gave the SAME figures in every case (the same arithmetic: an excluded key adds exact zeros):
      (2,2,33,65), key 64:    dq 3.306e-05 / dk 9.331e-05 'mixed', 3.306e-05 / 9.370e-05 'split', 3.516e-05 / 6.926e-05 'bf16x3',
                              1.118e-06 / 2.361e-06 'fp32';
      (2,2,100,200), key 199: dq 3.922e-05 / dk 2.119e-04 'mixed', 3.944e-05 / 2.129e-04 'split', 3.579e-05 / 2.001e-04 'bf16x3',
                              8.626e-07 / 2.844e-06 'fp32'."""
    Q, K, V, dO = operands(B, h, nq, nk)
    mask, empty = exclusion_case(name, B, h, nq, nk)
    want = attention_grads(Q, K, V, h, mask, dO)
    got = run(Q, K, V, dO, h, mask, policy)
    for t in got:
        assert not torch.isnan(t).any()
    o, lse, dq = got[0].cpu(), got[1].cpu(), got[2].cpu()
    if name.startswith("empty"):
        assert empty.any()
    assert (o[empty] == 0).all()
    assert (lse[empty] == -math.inf).all() and torch.isfinite(lse[~empty]).all()
    dq_rows = dq.view(B, nq, h, HD).permute(0, 2, 1, 3)                   # [B,h,q,32]
    assert (dq_rows[empty] == 0).all()
    allow = None
    kept = mask.expand(B, h, nq, nk).reshape(-1, nk)
    if bool((kept.sum(-1) == 1).all()) and bool((kept == kept[0]).all()):
        j = int(kept[0].nonzero())
        Kj, Vj = K[:, j:j + 1].contiguous(), V[:, j:j + 1].contiguous()
        plain, ref = run(Q, Kj, Vj, dO, h, None, policy), attention_grads(Q, Kj, Vj, h, None, dO)
        assert ref[2].abs().max() == 0 and ref[3].abs().max() == 0
        allow = {"dq": 2 * max_err(plain[2], ref[2]), "dk": 2 * max_err(plain[3], ref[3])}
        print(f"unmasked kernel on the kept key {j}: dq residue {allow['dq'] / 2:.3e}, dk residue {allow['dk'] / 2:.3e}")
    check(got, want, policy, name, allow)


@pytest.mark.parametrize("policy", POLICIES)
def test_prefix_key_mask_equals_truncated_keys(cuda, policy):
    """A prefix key mask per image gives the outputs of the unmasked call on K[b, :n_b], V[b, :n_b], within the forward bar."""
    from boosted_detr_amd import kernels as k
    B, h, nq, nk = 2, 2, 100, 200
    Q, K, V, dO = operands(B, h, nq, nk)
    lengths = (37, 130)
    mask = torch.zeros(B, 1, 1, nk, dtype=torch.bool)
    for b, n in enumerate(lengths):
        mask[b, ..., :n] = True
    o, lse = run(Q, K, V, dO, h, mask, policy)[:2]
    scale = 1.0 / math.sqrt(HD)
    for b, n in enumerate(lengths):
        with k.gemm_precision(policy):
            ob, lb = k.attention_fwd(dev(Q[b:b + 1]), dev(K[b:b + 1, :n]), dev(V[b:b + 1, :n]), h, scale)
        close(o[b:b + 1], ob, fwd_tol(policy), f"image {b} o")
        close(lse[b:b + 1], lb, fwd_tol(policy), f"image {b} lse")


# ----------------------------------------------------------------------------------------------- memory bounds
@pytest.mark.parametrize("policy", ["split", "fp32"])
@pytest.mark.parametrize("form", ["Bhqk", "B11k"])
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("B,h,nq,nk", [(2, 3, 130, 49), (2, 2, 33, 65)])
def test_masked_attention_inside_the_guard_arena(cuda, B, h, nq, nk, rule, form, policy):
    """Masked forward and backward with every operand - the mask as a read-only one - between 0xFF margins: a load past a mask
    row's end at the tensor's tail reads NaN (f32) or 'attend' (u8) and poisons a result; a store outside a result changes a margin."""
    from boosted_detr_amd import kernels as k
    Q, K, V, dO, mask, want = case(B, h, nq, nk, form, rule)
    scale = 1.0 / math.sqrt(HD)
    arena = _guard.Arena(cuda)
    with arena.armed(dev_modules=()):
        q, kk, v, do, m = (arena.place(t) for t in (Q, K, V, dO, mask))
        with k.gemm_precision(policy):
            o, lse = k.attention_fwd(q, kk, v, h, scale, mask=m)
            dq, dk, dv = k.attention_bwd(q, kk, v, o, do, lse, h, scale, mask=m)
    assert arena.verify() >= 5
    check((o, lse, dq, dk, dv), want, policy, f"guarded {rule} {form}")


# ----------------------------------------------------------------------------------------------- unfused path (head dim != 32)
def tape_core(Q, K, V, dO, h, mask):
    from boosted_detr_amd import ops
    from boosted_detr_amd.engine import Tape, recording
    q, kk, v = dev(Q), dev(K), dev(V)
    tape = Tape()
    with recording(tape):
        o = ops.attention_core(q, kk, v, h, mask=None if mask is None else dev(mask))
    grads = tape.backward({id(o): dev(dO)})
    torch.cuda.synchronize()
    return o, grads[id(q)], grads[id(kk)], grads[id(v)]


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("form", ["Bhqk", "B11k"])
@pytest.mark.parametrize("rule", RULES)
def test_unfused_path_takes_both_rules(cuda, rule, form, policy):
    """Head dim 16 runs batched GEMMs + softmax_rows with the element-wise mask kernel; a fully excluded row is included."""
    from boosted_detr_amd import kernels as k
    B, h, nq, nk, d = 2, 4, 50, 49, 16
    Q, K, V, dO = operands(B, h, nq, nk, d)
    mask = make_mask(rule, mask_shape(form, B, h, nq, nk), seed=21)
    if rule == "exclude":
        mask[0] = False                                                   # image 0 (form B11k) / its every row (Bhqk): no kept key
        mask[1, ..., :3] = True
    want = attention_grads(Q, K, V, h, mask, dO)
    with k.gemm_precision(policy):
        o, dq, dk, dv = tape_core(Q, K, V, dO, h, mask)
    for t in (o, dq, dk, dv):
        assert not torch.isnan(t).any()
    if rule == "exclude":
        assert (o[0] == 0).all() and (dq[0] == 0).all()
    close(o, want[0], fwd_tol(policy), "o")
    for name, g, w in zip(("dq", "dk", "dv"), (dq, dk, dv), want[2:]):
        close(g, w, bwd_tol(policy), name)


def test_fused_core_on_the_tape_returns_three_gradients(cuda):
    B, h, nq, nk = 2, 2, 33, 65
    Q, K, V, dO, mask, want = case(B, h, nq, nk, "B1qk", "multiply")
    o, dq, dk, dv = tape_core(Q, K, V, dO, h, mask)
    close(o, want[0], 1e-5, "o")
    for name, g, w in zip(("dq", "dk", "dv"), (dq, dk, dv), want[2:]):
        close(g, w, 2e-4, name)


# ----------------------------------------------------------------------------------------------- layers
WIDTH, HEADS, LN_EPS = 256, 8, 1e-3
# Layer bars (left to the author, reasoned from the pieces, error relative to max|want| like every bar here).  Forward: two Dense
# layers in series (test_linear_fwd's bar, 2e-5 each), the attention core (1e-5) and a LayerNorm whose rstd is of order 1 at these
# operand scales: 1e-4.  Gradients: the attention gradient bar (2e-4), the row chain's (2e-4, test_rowchain_gpu) and the GEMM
# gradient bar (6e-5) in series: 5e-4.  A parameter gradient that is zero up to round-off (the key bias: softmax is shift invariant
# under both rules) is measured against 1 % of the largest parameter gradient, as test_rowchain_gpu does.
LAYER_FWD_TOL, LAYER_BWD_TOL = 1e-4, 5e-4


def layer_reference(P, q, kv, v, mask, gout, with_ln):
    """fp64: projections -> masked core -> reshape WITHOUT a head permute -> OutputProjection (-> LayerNorm(q + .)).
    Dense kernels as the Variables hold them: [out, in]."""
    P = {n: t.detach().cpu().double().requires_grad_(True) for n, t in P.items()}
    q, kv, v = (t.detach().cpu().double().requires_grad_(True) for t in (q, kv, v))
    Qp, Kp, Vp = q @ P["Qk"].T + P["Qb"], kv @ P["Kk"].T + P["Kb"], v @ P["Vk"].T + P["Vb"]
    o, _ = attention_ref(Qp, Kp, Vp, HEADS, None if mask is None else mask.cpu())
    B, h, nq, d = o.shape
    y = o.reshape(B, nq, h * d) @ P["Ok"].T + P["Ob"]
    if with_ln:
        x = q + y
        mu, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
        y = (x - mu) / torch.sqrt(var + LN_EPS) * P["g"] + P["b"]
    y.backward(gout.detach().cpu().double())
    return y.detach(), {"q": q.grad, "k": kv.grad, "v": v.grad}, {n: t.grad for n, t in P.items()}


def layer_params(mha, attn=None):
    P = {"Qk": mha.QueryProjection.kernel, "Qb": mha.QueryProjection.bias, "Kk": mha.KeyProjection.kernel, "Kb": mha.KeyProjection.bias,
         "Vk": mha.ValueProjection.kernel, "Vb": mha.ValueProjection.bias, "Ok": mha.OutputProjection.kernel, "Ob": mha.OutputProjection.bias}
    if attn is not None:
        P.update({"g": attn.ln_gamma, "b": attn.ln_beta})
    return P


def run_layer(fn, variables, inputs, gout):
    from boosted_detr_amd.engine import Tape, join_side_stream, recording
    for var in variables:
        var.reset_grad()
    tape = Tape()
    with recording(tape):
        out = fn()
    grads = tape.backward({id(out): gout})
    join_side_stream()
    torch.cuda.synchronize()
    return out, {n: grads[id(t)] for n, t in inputs.items()}


def layer_masks(B, nq, nk):
    key_bool = torch.rand(B, 1, 1, nk, generator=torch.Generator().manual_seed(31)) < 0.6
    key_bool[..., 0] = True
    return {"key_bool": key_bool, "full_f32": make_mask("multiply", (B, HEADS, nq, nk), seed=32)}


@pytest.mark.parametrize("route", ["rowchain", "layers"])
@pytest.mark.parametrize("which", ["key_bool", "full_f32"])
@pytest.mark.parametrize("layer", ["MultiheadAttention", "AttentionBlock"])
def test_layers_take_the_mask(cuda, layer, which, route):
    """MultiheadAttention and AttentionBlock (training on a tape, dropout 0) at width 256, 8 heads, B = 2, q = 33, k = 65 against the
    fp64 restatement: outputs, the gradients of the four kernels (and biases, LayerNorm) and of the three inputs; once on the
    row-chain route ('split' policy, attention_then) and once layer by layer."""
    from boosted_detr_amd import kernels as k, ops, transformers as T
    from boosted_detr_amd.engine import bump_weights_version
    B, nq, nk = 2, 33, 65
    keep = (T.AttentionBlock.dropout_rate, T.FeedForwardBlock.dropout_rate, ops.ROWCHAIN[0])
    try:
        T.AttentionBlock.dropout_rate = T.FeedForwardBlock.dropout_rate = 0.0
        q, kv, v = dev(rnd(B, nq, WIDTH, seed=1)), dev(rnd(B, nk, WIDTH, seed=2)), dev(rnd(B, nk, WIDTH, seed=3))
        gout = dev(rnd(B, nq, WIDTH, seed=4))
        mask = dev(layer_masks(B, nq, nk)[which])
        ops.ROWCHAIN[0] = route == "rowchain"
        with k.gemm_precision("split"):
            if layer == "MultiheadAttention":
                mha = T.MultiheadAttention(HEADS, WIDTH // HEADS, name="M", seed=5)
                mha([q, kv, v], training=True)                                       # build
                attn, variables = None, mha.variables
                fn = lambda: mha([q, kv, v], attention_mask=mask, training=True)
            else:
                attn = T.AttentionBlock(HEADS, name="A", seed=5)
                attn([q, kv, v], training=True)
                mha, variables = attn.AttentionLayer, attn.variables
                fn = ((lambda: T.attention_then(attn, None, [q, kv, v], True, attention_mask=mask)) if route == "rowchain"
                      else (lambda: attn([q, kv, v], attention_mask=mask, training=True)))
            for var in variables:
                if var.value.dim() == 1:                                             # biases / gamma / beta away from 0 / 1
                    var.value.add_(dev(rnd(*var.value.shape, seed=len(var.name), scale=0.2)))
            bump_weights_version()
            assert route != "rowchain" or layer != "AttentionBlock" or ops.rowchain_active(WIDTH)
            out, gin = run_layer(fn, variables, {"q": q, "k": kv, "v": v}, gout)
        P = layer_params(mha, attn)
        want_out, want_in, want_p = layer_reference({n: var.value for n, var in P.items()}, q, kv, v, mask, gout, attn is not None)
        close(out, want_out, LAYER_FWD_TOL, "out")
        for n in ("q", "k", "v"):
            close(gin[n], want_in[n], LAYER_BWD_TOL, "d" + n)
        top = max(float(t.abs().max()) for t in want_p.values())
        for n, var in P.items():
            assert var.grad is not None, n
            w = want_p[n]
            err = (var.grad.cpu().double() - w).abs().max().item()
            bar = LAYER_BWD_TOL * max(float(w.abs().max()), 1e-2 * top)
            print(f"{n}: max err {err:.3e} (bar {bar:.3e})")
            assert err <= bar, f"{n}: max err {err:.3e} > {bar:.3e}"
    finally:
        T.AttentionBlock.dropout_rate, T.FeedForwardBlock.dropout_rate, ops.ROWCHAIN[0] = keep


def _encoder(seed):
    from boosted_detr_amd import transformers as T
    return T.EncoderBlock(HEADS, name="E", seed=seed)


def _decoder(seed):
    from boosted_detr_amd import transformers as T
    return T.DecoderBlock(HEADS, name="D", seed=seed)


@pytest.mark.parametrize("training", [False, True])
def test_encoder_block_keyword(cuda, training):
    """EncoderBlock.call(attention_mask=) equals the composition of its pieces given the same mask; None equals no keyword, bit for bit."""
    from boosted_detr_amd import kernels as k, ops, transformers as T
    B, T_ = 2, 65
    keep = (T.AttentionBlock.dropout_rate, T.FeedForwardBlock.dropout_rate)
    try:
        T.AttentionBlock.dropout_rate = T.FeedForwardBlock.dropout_rate = 0.0
        x, pos = dev(rnd(B, T_, WIDTH, seed=1)), dev(rnd(T_, WIDTH, seed=2))
        mask = dev(layer_masks(B, T_, T_)["key_bool"])
        with k.gemm_precision("split"):
            blk = _encoder(3)
            plain = blk([x, pos], training=training)
            none = blk([x, pos], training=training, attention_mask=None)
            assert torch.equal(plain, none)
            got = blk([x, pos], training=training, attention_mask=mask)
            qk = ops.add_bcast(x, pos)
            want = T.attention_then(blk.SelfAttentionBlock, blk.FeedForwardBlock, [qk, qk, x], training, attention_mask=mask)
            pieces = blk.FeedForwardBlock([blk.SelfAttentionBlock([qk, qk, x], attention_mask=mask, training=False)], training=False)
        assert torch.equal(got, want)
        assert not torch.equal(got, plain)
        close(got, pieces, 3e-5, "block against its pieces, layer by layer")            # (test_rowchain_gpu's forward bar between the routes)
        enc = T.ImageEncoderAttention(2, HEADS, seed=4)
        img = dev(rnd(B, 5, 13, WIDTH, seed=5))
        with k.gemm_precision("split"):
            a = enc([img], training=training)[0]
            b = enc([img], training=training, attention_mask=None)[0]
            c = enc([img], training=training, attention_mask=mask)[0]
            y = ops.reshape(img, (B, T_, WIDTH))
            for e in enc.EncoderBlocks:
                y = e([y, enc.positional_encoding], training=training, attention_mask=mask)
        assert torch.equal(a, b) and not torch.equal(a, c)
        assert torch.equal(c.view(B, T_, WIDTH), y)
    finally:
        T.AttentionBlock.dropout_rate, T.FeedForwardBlock.dropout_rate = keep


@pytest.mark.parametrize("training", [False, True])
def test_decoder_block_keywords(cuda, training):
    """DecoderBlock.call(self_attention_mask=, joint_attention_mask=) and DecoderBlock_NoSelfAttention.call(joint_attention_mask=)
    equal the composition of their pieces; None equals no keyword, bit for bit."""
    from boosted_detr_amd import kernels as k, transformers as T
    B, N, T_ = 2, 33, 65
    keep = (T.AttentionBlock.dropout_rate, T.FeedForwardBlock.dropout_rate)
    try:
        T.AttentionBlock.dropout_rate = T.FeedForwardBlock.dropout_rate = 0.0
        ev, ek, df = dev(rnd(B, T_, WIDTH, seed=1)), dev(rnd(B, T_, WIDTH, seed=2)), dev(rnd(B, N, WIDTH, seed=3))
        joint = dev(layer_masks(B, N, T_)["key_bool"])
        self_mask = dev(make_mask("multiply", (1, 1, N, N), seed=33))
        inputs = [ev, df, ek, df]
        with k.gemm_precision("split"):
            blk = _decoder(6)
            plain = blk(inputs, training=training)
            assert torch.equal(plain, blk(inputs, training=training, self_attention_mask=None, joint_attention_mask=None))
            got = blk(inputs, training=training, self_attention_mask=self_mask, joint_attention_mask=joint)
            x = T.attention_then(blk.SelfAttentionBlock, None, [df, df, df], training, attention_mask=self_mask)
            want = T.attention_then(blk.JointAttentionBlock, blk.FeedForwardBlock, [x, ek, ev], training, attention_mask=joint)
            only_joint = blk(inputs, training=training, joint_attention_mask=joint)
            only_self = blk(inputs, training=training, self_attention_mask=self_mask)
            first = T.DecoderBlock_NoSelfAttention(HEADS, name="D0", seed=7)
            p0 = first(inputs, training=training)
            assert torch.equal(p0, first(inputs, training=training, joint_attention_mask=None))
            g0 = first(inputs, training=training, joint_attention_mask=joint)
            w0 = T.attention_then(first.JointAttentionBlock, first.FeedForwardBlock, [df, ek, ev], training, attention_mask=joint)
        assert torch.equal(got, want) and torch.equal(g0, w0)
        for other in (plain, only_joint, only_self):
            assert not torch.equal(got, other)
        assert not torch.equal(g0, p0)
    finally:
        T.AttentionBlock.dropout_rate, T.FeedForwardBlock.dropout_rate = keep


# ----------------------------------------------------------------------------------------------- argument checks
def test_bad_masks_raise_value_error_before_a_launch(cuda):
    from boosted_detr_amd import kernels as k, ops
    B, h, nq, nk = 2, 2, 33, 65
    Q, K, V, dO = operands(B, h, nq, nk)
    q, kk, v = dev(Q), dev(K), dev(V)
    scale = 1.0 / math.sqrt(HD)
    o, lse = k.attention_fwd(q, kk, v, h, scale)
    good = torch.ones(B, h, nq, nk, device="cuda")
    bad = {
        "3-D": torch.ones(B, nq, nk, device="cuda"),
        "wrong key length": torch.ones(B, 1, 1, nk - 1, device="cuda"),
        "key axis of 1": torch.ones(B, 1, 1, 1, device="cuda"),
        "batch neither 1 nor full": torch.ones(3, 1, 1, nk, device="cuda"),
        "head neither 1 nor full": torch.ones(1, 3, 1, nk, device="cuda"),
        "query neither 1 nor full": torch.ones(1, 1, nq - 1, nk, device="cuda"),
        "float64": good.double(),
        "int64": good.long(),
        "non-contiguous": torch.ones(B, h, nk, nq, device="cuda").transpose(2, 3),
        "cpu mask": torch.ones(B, h, nq, nk),
        "cpu bool mask": torch.ones(B, 1, 1, nk, dtype=torch.bool),
    }
    calls = []
    real = k._lib.lib

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(real(), name)

    k._lib.lib = lambda: Spy()
    try:
        for what, m in bad.items():
            with pytest.raises(ValueError):
                k.attention_fwd(q, kk, v, h, scale, mask=m)
            with pytest.raises(ValueError):
                k.attention_bwd(q, kk, v, o, dev(dO), lse, h, scale, mask=m)
            with pytest.raises(ValueError):
                ops.attention_core(q, kk, v, h, mask=m)
            with pytest.raises(ValueError):
                ops.attention_core(q[..., :32], kk[..., :32], v[..., :32], h, mask=m)      # head dim 16: the unfused path
            assert calls == [], (what, calls)
    finally:
        k._lib.lib = real
    k.attention_fwd(q, kk, v, h, scale, mask=good)


def test_c_entry_points_refuse_bad_mask_arguments(cuda):
    """Null mask, unknown mode, negative strides, size x stride overflow: a status and bdetr_last_error before any launch."""
    from boosted_detr_amd import _lib
    B, h, nq, nk = 1, 1, 4, 4
    q = torch.zeros(B, nq, 32, device="cuda")
    o, lse = torch.full((B, h, nq, 32), 7.0, device="cuda"), torch.full((B, h, nq), 7.0, device="cuda")
    m = torch.ones(B, h, nq, nk, device="cuda")
    L = _lib.lib()
    p = lambda t: t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream

    def fwd(mask, sb, sh, sq, mode):
        return L.bdetr_attention_masked_fwd(p(q), p(q), p(q), p(o), p(lse), B, h, nq, nk, 1.0, mask, sb, sh, sq, mode, st)

    def bwd(mask, sb, sh, sq, mode):
        return L.bdetr_attention_masked_bwd(p(q), p(q), p(q), p(o), p(o), p(lse), p(o), p(o), p(o), p(lse), B, h, nq, nk, 1.0, mask, sb, sh, sq, mode, st)

    big = 2 ** 62
    for f in (fwd, bwd):
        for args in ((None, 0, 0, nk, 1), (p(m), 0, 0, nk, 0), (p(m), 0, 0, nk, 3), (p(m), -1, 0, nk, 1), (p(m), 0, -4, nk, 2),
                     (p(m), 0, 0, -nk, 1), (p(m), 0, 0, big, 1), (p(m), 0, 0, 2 ** 63 - 1, 2)):
            assert f(*args) != 0, args
    torch.cuda.synchronize()
    assert (o == 7.0).all() and (lse == 7.0).all()                       # nothing was launched
    assert fwd(p(m), 0, 0, nk, 1) == 0
