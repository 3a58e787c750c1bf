"""Attention masks without a GPU: the fp64 reference of the two rules checks itself, and the new C entry points are declared,
bound and exported (include/bdetr.h K32-K34)."""
import math
import re
from pathlib import Path

import torch

from _attention_mask_ref import attention_grads, attention_ref, probabilities, split_heads

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("bdetr_attention_masked_fwd", "bdetr_attention_masked_bwd")


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def operands(B=2, h=3, nq=7, nk=11, d=4):
    return rnd(B, nq, h * d, seed=1), rnd(B, nk, h * d, seed=2), rnd(B, nk, h * d, seed=3), rnd(B, h, nq, d, seed=4), h


def plain(Q, K, V, heads):
    Qh, Kh, Vh, scale = split_heads(Q, K, V, heads)
    s = (Qh @ Kh) * scale
    return torch.softmax(s, -1) @ Vh, torch.logsumexp(s, -1)


def test_all_ones_and_all_true_masks_are_plain_attention():
    Q, K, V, dO, h = operands()
    want = attention_grads(Q, K, V, h, None, dO)
    o, lse = plain(Q, K, V, h)
    assert torch.equal(want[0], o) and torch.equal(want[1], lse)
    for shape in ((2, 1, 1, 11), (1, 1, 7, 11), (2, 3, 7, 11)):
        for mask in (torch.ones(shape, dtype=torch.float32), torch.ones(shape, dtype=torch.bool)):
            got = attention_grads(Q, K, V, h, mask, dO)
            for g, w in zip(got, want):
                assert torch.allclose(g, w, rtol=0, atol=1e-14), (shape, mask.dtype)


def test_bool_prefix_key_mask_is_attention_on_truncated_keys():
    Q, K, V, dO, h = operands()
    lengths = (4, 9)
    mask = torch.zeros(2, 1, 1, 11, dtype=torch.bool)
    for b, n in enumerate(lengths):
        mask[b, ..., :n] = True
    o, lse, dQ, dK, dV = attention_grads(Q, K, V, h, mask, dO)
    for b, n in enumerate(lengths):
        w = attention_grads(Q[b:b + 1], K[b:b + 1, :n], V[b:b + 1, :n], h, None, dO[b:b + 1])
        assert torch.allclose(o[b:b + 1], w[0], rtol=0, atol=1e-14) and torch.allclose(lse[b:b + 1], w[1], rtol=0, atol=1e-14)
        assert torch.allclose(dQ[b:b + 1], w[2], rtol=0, atol=1e-14)
        assert torch.allclose(dK[b:b + 1, :n], w[3], rtol=0, atol=1e-14) and torch.allclose(dV[b:b + 1, :n], w[4], rtol=0, atol=1e-14)
        assert (dK[b, n:] == 0).all() and (dV[b, n:] == 0).all()          # an excluded key gets no gradient


def test_multiply_rule_row_dot_identity_and_closed_form_backward():
    """sum_k P_k M_k (dO . V_k) = dO . O, so dS = P (M dP - D) scale with D = rowdot(dO, O): the closed form the kernels use equals autograd."""
    Q, K, V, dO, h = operands()
    M = rnd(2, 3, 7, 11, seed=5).float() * 1.5
    M[rnd(2, 3, 7, 11, seed=6) > 0.5] = 0.0                               # zeros, negatives, values above 1
    assert (M == 0).any() and (M < 0).any() and (M > 1).any()
    o, lse, dQ, dK, dV = attention_grads(Q, K, V, h, M, dO)
    Qh, Kh, Vh, scale = split_heads(Q, K, V, h)
    s = (Qh @ Kh) * scale
    P, PM, lse2 = probabilities(s, M)
    assert torch.equal(lse, torch.logsumexp(s, -1)) and torch.equal(lse, lse2)        # lse: the unmasked scores
    dPu = dO @ Vh.transpose(-1, -2)
    D = (dO * o).sum(-1)
    assert torch.allclose((PM * dPu).sum(-1), D, rtol=0, atol=1e-13)
    dS = P * (M.double() * dPu - D[..., None]) * scale
    B, nq, nk, d = 2, 7, 11, 4
    merge = lambda t, n: t.permute(0, 2, 1, 3).reshape(B, n, h * d)      # [B,h,n,d] -> [B,n,h*d]
    assert torch.allclose(merge(dS @ Kh.transpose(-1, -2), nq), dQ, rtol=0, atol=1e-13)
    assert torch.allclose(merge(dS.transpose(-1, -2) @ Qh, nk), dK, rtol=0, atol=1e-13)
    assert torch.allclose(merge(PM.transpose(-1, -2) @ dO, nk), dV, rtol=0, atol=1e-13)


def test_empty_row_gives_zeros_and_no_nan():
    Q, K, V, dO, h = operands()
    mask = rnd(2, 3, 7, 11, seed=7) > 0
    mask[0, 1, 2] = False
    mask[1, :, 6] = False
    o, lse, dQ, dK, dV = attention_grads(Q, K, V, h, mask, dO)
    for t in (o, dQ, dK, dV):
        assert torch.isfinite(t).all()
    assert not torch.isnan(lse).any()
    assert (o[0, 1, 2] == 0).all() and (o[1, :, 6] == 0).all()
    assert lse[0, 1, 2] == -math.inf and (lse[1, :, 6] == -math.inf).all()
    assert torch.isfinite(lse).sum() == lse.numel() - 4
    d = 4
    assert (dQ[0, 2, d:2 * d] == 0).all() and (dQ[1, 6] == 0).all()       # head 1 of image 0, every head of image 1
    # the empty rows contribute nothing: the other rows' results are those of a call without them
    keep_rows = [i for i in range(7) if i != 6]
    w = attention_grads(Q[1:, keep_rows], K[1:], V[1:], h, mask[1:, :, keep_rows], dO[1:, :, keep_rows])
    assert torch.allclose(dK[1:], w[3], rtol=0, atol=1e-14) and torch.allclose(dV[1:], w[4], rtol=0, atol=1e-14)


def test_mask_without_gradient():
    Q, K, V, dO, h = operands()
    M = torch.ones(2, 1, 1, 11, dtype=torch.float32)
    o, _ = attention_ref(Q, K, V, h, M)
    assert not o.requires_grad and not M.requires_grad


def test_masked_entry_points_are_declared_bound_and_exported():
    import __graft_entry__
    __graft_entry__.build()
    from boosted_detr_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "bdetr.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(bdetr_[a-z0-9_]+)\s*\(", text))
    h = _lib.lib()
    for s in NEW_SYMBOLS + ("bdetr_attention_mask_apply",):
        assert s in declared, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(h, s), s
    nargs = {s: len(_lib.SIGNATURES[s][1]) for s in _lib.SIGNATURES}
    # the operands of the unmasked pair, then mask, three strides and the mode
    assert nargs["bdetr_attention_masked_fwd"] == nargs["bdetr_attention_fwd"] + 5
    assert nargs["bdetr_attention_masked_bwd"] == nargs["bdetr_attention_bwd"] + 5
    assert h.bdetr_abi_version() == 8
