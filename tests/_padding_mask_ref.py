"""Shared reference of the padding-mask tests (include/bdetr.h K35; the batch key `valid_region`).

token_keep      the integer rule in NumPy int64, written from the header's two inequalities (not from the package's host function).
MaskedNet       oracle.detr_oracle.Net with `mha` overridden: the scores of excluded keys are filled with -inf before the softmax, for
                the encoder's self-attention and every decoder block's attention over the image - decided by the layer's NAME, not by
                the key length.  Everything else (backbone, heads, matcher, loss, autograd) is the unchanged oracle code, reached
                through O.forward(net, batch, training).
The model case  CONFIG1 with 2 + 2 layers, batch 2, regions [[0,0,224,224],[16,0,120,150]]: image 1 keeps rows 0-3 and columns 0-4 of
                the 7 x 7 grid (20 of 49 tokens); its top edge 16 sits exactly on a token centre (inclusive), its bottom 136 excludes
                the centre at 144.
References are computed once per process and shared (functools.lru_cache); nobody writes into them."""
import dataclasses
import functools
import math
import re

import numpy as np
import torch

from oracle import detr_oracle as O

MODEL_REGIONS = np.array([[0, 0, 224, 224], [16, 0, 120, 150]], np.int32)
MODEL_KEPT = (49, 20)


def token_keep(region, h, w, r, c):
    """bool [B, r*c]: token (i, j) at i*c + j kept iff 2 r top <= (2i+1) h < 2 r (top+height) and 2 c left <= (2j+1) w < 2 c (left+width)."""
    region = np.asarray(region, np.int64).reshape(-1, 4)
    out = np.zeros((region.shape[0], r * c), bool)
    for b, (top, left, height, width) in enumerate(region.tolist()):
        for i in range(r):
            if not (2 * r * top <= (2 * i + 1) * h < 2 * r * (top + height)):
                continue
            for j in range(c):
                out[b, i * c + j] = 2 * c * left <= (2 * j + 1) * w < 2 * c * (left + width)
    return out


_ENCODER_SELF = re.compile(r"^ImageEncoderAttention[^/]*/.*SelfAttentionBlock")


def masks_keys(name: str) -> bool:
    """Does the attention layer of this name attend over the image tokens as keys?"""
    return bool(_ENCODER_SELF.match(name)) or "JointAttentionBlock" in name


class MaskedNet(O.Net):
    def __init__(self, cfg, params, keep, **kw):
        super().__init__(cfg, params, **kw)
        keep = np.asarray(keep, bool)
        assert keep.any(axis=1).all(), "an image without a kept token: the -inf fill would leave an empty softmax row"
        self.keep = torch.from_numpy(keep)                # [B, T]
        self.masked_layers = []

    def mha(self, q, k, v, name, heads):
        """O.Net.mha (transformers.py:68-102) with the exclusion rule in front of the softmax."""
        B, nq, dq = q.shape
        d = dq // heads
        Q = self.dense(q, f"{name}/QueryProjection").reshape(B, nq, heads, d).permute(0, 2, 1, 3)
        Kt = self.dense(k, f"{name}/KeyProjection").reshape(B, k.shape[1], heads, d).permute(0, 2, 3, 1)
        V = self.dense(v, f"{name}/ValueProjection").reshape(B, v.shape[1], heads, d).permute(0, 2, 1, 3)
        scale = torch.tensor(1.0 / math.sqrt(float(d)), dtype=torch.float32).to(self.dtype)
        s = (Q @ Kt) * scale
        if masks_keys(name):
            assert k.shape[1] == self.keep.shape[1], (name, k.shape, self.keep.shape)
            s = s.masked_fill(~self.keep[:, None, None, :], float("-inf"))
            self.masked_layers.append(name)
        o = (torch.softmax(s, dim=-1) @ V).reshape(B, nq, heads * d)
        return self.dense(o, f"{name}/OutputProjection")


def keep_of(cfg, batch, regions):
    h, w = np.asarray(batch["image"]).shape[1:3]
    r, c = cfg.feature_hw
    return token_keep(regions, h, w, r, c)


def step_grads(cfg, params, batch, keep=None, dtype=torch.float32):
    """O.train_step_grads' five lines around MaskedNet (keep=None: around O.Net, i.e. O.train_step_grads itself)."""
    net = O.Net(cfg, params, dtype=dtype, requires_grad=True) if keep is None else MaskedNet(cfg, params, keep, dtype=dtype, requires_grad=True)
    out = O.forward(net, batch, training=True)
    out.loss_vector.sum().backward()
    grads = {k: (v.grad.detach().numpy() if v.grad is not None else np.zeros(tuple(v.shape), np.float32))
             for k, v in net.p.items() if v.requires_grad}
    return out, grads


def match_matrix(out, B, M):
    """int [B, M] in the layout of loss_fn.last_match: query of ground truth m, -1 where there is none."""
    want = -np.ones((B, M), np.int64)
    for b, (rows, cols) in enumerate(out.loss.matches):
        want[b, rows] = cols
    return want


@functools.lru_cache(maxsize=None)
def model_case():
    cfg = dataclasses.replace(O.CONFIG1, num_encoder_blocks=2, num_decoder_blocks=2)
    batch = O.make_batch(cfg, 2, 20, seed=1234, num_objects=[3, 7])
    return cfg, batch, O.make_params(cfg, seed=0)


@functools.lru_cache(maxsize=None)
def boosted_case():
    """test_model_gpu.test_boosted_three_learners' configuration; its images are 224 x 224, so the regions are the model case's."""
    cfg = O.Config(num_decoder_blocks=3, boosted=True)
    batch = O.make_batch(cfg, 2, 20, seed=77, num_objects=[5, 2])
    return cfg, batch, O.make_params(cfg, seed=0)


@functools.lru_cache(maxsize=None)
def reference(case: str, masked: bool, bits: int):
    """(StepOut, grads) of one training step of the case ('model' / 'boosted') in fp32 or fp64, with or without the mask."""
    cfg, batch, params = model_case() if case == "model" else boosted_case()
    keep = keep_of(cfg, batch, MODEL_REGIONS) if masked else None
    return step_grads(cfg, params, batch, keep, torch.float32 if bits == 32 else torch.float64)


def grad_rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))
