"""fp64 restatement of the two attention-mask rules (include/bdetr.h K32 / K33), plain torch, gradients from autograd.

    o, lse = attention_ref(Q, K, V, heads, mask)        Q [B,q,h*d], K / V [B,k,h*d]  ->  o [B,h,q,d], lse [B,h,q]

The output layout is the one transformers.py:100 reshapes without a permute.  mask: None, or [B or 1, h or 1, q or 1, k]:
  float mask M (multiply, the reference's rule): P = softmax(scale Q K^T) over ALL keys, o = (P * M) V, lse = logsumexp of the
      unmasked scaled scores; M may hold anything, nothing is renormalised.
  bool mask (exclusion, the project's own rule): True attends; an excluded key has score -inf; lse runs over the kept keys; a row
      with no kept key is handled explicitly (never through NaN): o = 0, lse = -inf, and it passes no gradient on.
The mask is a constant.  Inputs that are fp64 leaves with requires_grad collect gradients through o.backward(dO)."""
import math

import torch


def split_heads(Q, K, V, heads):
    B, nq, D = Q.shape
    nk, d = K.shape[1], D // heads
    Qh = Q.view(B, nq, heads, d).permute(0, 2, 1, 3)
    Kh = K.view(B, nk, heads, d).permute(0, 2, 3, 1)
    Vh = V.view(B, nk, heads, d).permute(0, 2, 1, 3)
    return Qh, Kh, Vh, 1.0 / math.sqrt(float(d))


def probabilities(s, mask):
    """(P, PM, lse) of scaled scores s [B,h,q,k]: the softmax, what multiplies V, and the log-sum-exp."""
    if mask is None:
        P = torch.softmax(s, -1)
        return P, P, torch.logsumexp(s, -1)
    if mask.dtype == torch.bool:
        keep = mask.expand(s.shape)
        some = keep.any(-1, keepdim=True)
        neg = torch.full_like(s, -math.inf)
        kept = torch.where(keep, s, neg)
        safe = torch.where(some, kept, torch.zeros_like(s))            # an empty row: any finite scores, its result is replaced below
        P = torch.where(keep & some, torch.softmax(safe, -1), torch.zeros_like(s))
        lse = torch.where(some.squeeze(-1), torch.logsumexp(safe, -1), neg[..., 0])
        return P, P, lse
    P = torch.softmax(s, -1)
    return P, P * mask.double(), torch.logsumexp(s, -1)


def attention_ref(Q, K, V, heads, mask=None):
    Qh, Kh, Vh, scale = split_heads(Q.double(), K.double(), V.double(), heads)
    s = (Qh @ Kh) * scale
    _, PM, lse = probabilities(s, mask)
    return PM @ Vh, lse


def attention_grads(Q, K, V, heads, mask, dO):
    """(o, lse, dQ, dK, dV), all fp64 and detached."""
    Qd, Kd, Vd = (t.detach().double().clone().requires_grad_(True) for t in (Q, K, V))
    o, lse = attention_ref(Qd, Kd, Vd, heads, mask)
    o.backward(dO.double())
    return o.detach(), lse.detach(), Qd.grad, Kd.grad, Vd.grad
