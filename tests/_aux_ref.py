"""CPU reference of DETR's auxiliary decoder losses (model.py:179-186 with ``use_intermediate_losses`` on); not a test.

Composes oracle.detr_oracle.Net's primitives the way ``forward()``'s non-boosted branch does, with ``net.heads(dec, "", True)`` and
``matching_loss`` behind EVERY decoder block.  ``Net.bn`` computes ``new_moving`` from the moving statistics it finds in ``net.p`` on every
call, so between the blocks the heads' ``new_moving`` entries are copied into ``net.p`` (under no_grad): the L updates then chain as
Keras' do when the shared heads are called L times in one step."""
from dataclasses import dataclass, field
from typing import Dict, List

import numpy as np
import torch

from oracle import detr_oracle as O

HEAD_BN = ("CategoryPredictionHead/BatchNorm", "AttributePredictionHead/BatchNorm", "BoxPredictionHead/BatchNorm")
HEAD_MOVING = tuple(f"{h}/{s}" for h in HEAD_BN for s in ("moving_mean", "moving_variance"))
LOGIT_KEYS = ("CategoryPredictionHead/logits", "AttributePredictionHead/logits", "BoxPredictionHead/logits")


@dataclass
class AuxOut:
    layers: List[O.StepOut]                       # per decoder block: predictions, .loss (LossOut), .probes (the three heads' logits)
    loss_vector: torch.Tensor                     # [B]: sum over the blocks of the per-image total loss
    metrics: Dict[str, torch.Tensor]              # the four loss metrics summed over the blocks, IOU of the last block
    new_moving: Dict[str, torch.Tensor]           # every BatchNorm's moving statistics after the step (the heads': L chained updates)
    head_means: Dict[str, List[torch.Tensor]] = field(default_factory=dict)      # per head BatchNorm: the L per-block batch means / variances
    head_vars: Dict[str, List[torch.Tensor]] = field(default_factory=dict)

    def matches(self, l: int, B: int, M: int) -> np.ndarray:
        """int32 [B, M] match vector of block l (prediction index per object, -1 for padding rows)."""
        want = -np.ones((B, M), np.int32)
        for b, (r, c) in enumerate(self.layers[l].loss.matches):
            want[b, r] = c
        return want


def forward_aux(net: O.Net, batch) -> AuxOut:
    cfg = net.cfg
    assert not cfg.boosted
    image = torch.from_numpy(np.asarray(batch["image"]))
    x = net.resnet50(net.image_prep(image), True)
    feat = net.neck(x, True)
    cat_t, att_t = O.tokens_to_hot(batch["category"], batch["attribute"], cfg.num_categories, cfg.num_attributes, net.dtype)
    bbox = torch.from_numpy(np.asarray(batch["bbox"])).to(net.dtype)
    num_objects = np.asarray(batch["num_objects"])
    box_w = 0.0 if cfg.classification_only else O.DEFAULT_BOX_WEIGHT
    enc, pos = net.image_encoder(feat, "ImageEncoderAttention", cfg.num_encoder_blocks, True)
    value, dec, key = net.decoder_prep(enc, pos)
    original = {k: net.p[k] for k in HEAD_MOVING}
    layers, means, variances = [], {h: [] for h in HEAD_BN}, {h: [] for h in HEAD_BN}
    plain_bn = net.bn

    def recording_bn(x, name, eps, training, channel_dim=1):
        if name in HEAD_BN:                       # the batch statistics each call of a shared head folds into its moving statistics
            dims = [d for d in range(x.dim()) if d != channel_dim]
            means[name].append(x.detach().mean(dim=dims))
            variances[name].append(x.detach().var(dim=dims, unbiased=False))
        return plain_bn(x, name, eps, training, channel_dim)

    net.bn = recording_bn
    try:
        for i in range(cfg.num_decoder_blocks):
            dec = net.decoder_block(i, value, dec, key, True)
            cat, att, box = net.heads(dec, "", True)
            lo = O.matching_loss(cat_t, att_t, bbox, num_objects, cat, att, box, attribute_weight=cfg.attribute_weight, box_weight=box_w)
            layers.append(O.StepOut(cat, att, box, loss=lo, loss_vector=lo.total, probes={k: net.probes[k] for k in LOGIT_KEYS}))
            with torch.no_grad():
                for k in HEAD_MOVING:             # the next call of the shared head starts from what this one left
                    net.p[k] = net.new_moving[k]
    finally:
        del net.bn
        for k, v in original.items():
            net.p[k] = v
    metrics = {name: sum(getattr(s.loss, attr) for s in layers)
               for name, attr in (("Category_Loss", "category"), ("Attribute_Loss", "attribute"), ("Box_Loss", "box"), ("Existence_Loss", "exist"))}
    metrics["IOU"] = layers[-1].loss.iou
    return AuxOut(layers, sum(s.loss.total for s in layers), metrics, dict(net.new_moving), means, variances)


def train_step_grads(cfg: O.Config, params, batch, dtype=torch.float32):
    """(AuxOut, {name: gradient of sum_b sum_l loss}) - oracle.train_step_grads for the auxiliary-loss step."""
    net = O.Net(cfg, params, dtype=dtype, requires_grad=True)
    out = forward_aux(net, batch)
    out.loss_vector.sum().backward()
    grads = {k: (v.grad.detach().numpy() if v.grad is not None else np.zeros(tuple(v.shape), np.float32)) for k, v in net.p.items() if v.requires_grad}
    return out, grads


# the smallest model that has every structure: block 0 without self-attention, blocks 1-2 with it
SMALL_CFG = O.Config(image_size=(96, 96), num_encoder_blocks=1, num_decoder_blocks=3)
SMALL_BATCH_ARGS = dict(batch=2, max_objects=20, num_objects=[3, 7])
