"""Hungarian matcher + set criterion on the GPU.

Mirrors /root/reference/ModelComponents/losses_and_metrics.py: default weights (8-11),
MatchingLoss (75-161), MatchingMetric (164-192), MatchingMask (195-212), CostArray (215-225),
MatchingAssignment (228-251).  The reference builds [B,M,N,C] broadcast tensors and hops to the
host for scipy; here one kernel builds the [B,M,N] cost matrix, one workgroup per image solves
the assignment exactly in LDS (csrc/matcher.hip), and one kernel reduces the masked losses and
writes the sparse gradient - no host synchronisation anywhere.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import kernels as K
from .engine import Layer, current_tape

DEFAULT_CATEGORY_WEIGHT = 1000.0
DEFAULT_BOX_WEIGHT = 1.0
DEFAULT_ATTRIBUTE_WEIGHT = 100.0
DEFAULT_EXIST_WEIGHT = 100.0


class MatchingAssignment(Layer):
    """Bipartite assignment.  Returns the match vector (int32 [B,M], prediction index per object
    or -1); ``mask()`` expands it to the reference's {0,1} mask [B,M,N]."""

    def __init__(self, name="MatchingAssignment", **kwargs):
        super().__init__(name=name, **kwargs)
        self.built = True

    def call(self, cost_array, num_objects, training=False):
        return K.lsa(cost_array, num_objects)

    def __call__(self, cost_array, num_objects, **kw):
        return self.call(cost_array, num_objects)

    @staticmethod
    def mask(match, num_preds):
        return K.match_to_mask(match, num_preds)

    @staticmethod
    def validate(match, num_objects, num_preds):
        """scipy raises ValueError for NaN/-inf or infeasible matrices; the kernel leaves such rows
        at -1.  This check synchronises, so the training loop only calls it when asked to."""
        m = match.cpu().numpy()
        n = num_objects.cpu().numpy()
        for b in range(m.shape[0]):
            want = min(int(n[b]), num_preds, m.shape[1])      # the kernel clamps num_objects to the M padded rows
            if (m[b] >= 0).sum() != want:
                raise ValueError("cost matrix is infeasible or contains invalid numeric entries")


class MatchingMask(Layer):
    def __init__(self, name="MatchingMask", **kwargs):
        super().__init__(name=name, **kwargs)
        self.MatchingAssignment = MatchingAssignment()
        self.built = True

    def __call__(self, inputs, **kw):
        matching_costs, num_objects = inputs
        match = self.MatchingAssignment(matching_costs, num_objects)
        # the reference also returns `assigned_predictions` (max of the mask over objects, 206-207); the
        # loss kernel derives it from the match vector, so only the mask and the vector are returned
        return MatchingAssignment.mask(match, matching_costs.shape[-1]), match


class MatchingLoss(Layer):
    """``call([y_true, y_pred])`` with y_true = [category_ids int32 [B,M], attribute multi-hot
    [B,M,A], bbox [B,M,4], num_objects int32 [B]] and y_pred = [cat [B,N,C], att [B,N,A], box
    [B,N,4]].  Returns (losses, metrics) exactly like the reference: losses = [total, category,
    attribute, box, exist] (each [B]) and metrics = [masked_iou [B]].  When a Tape is recording,
    the gradient of sum_b total_b w.r.t. the three prediction tensors is registered on it."""

    def __init__(self, name="MatchingLoss", category_weight=None, box_weight=None, attribute_weight=None,
                 exist_weight=None, **kwargs):
        super().__init__(name=name, **kwargs)
        self.category_weight = float(DEFAULT_CATEGORY_WEIGHT if category_weight is None else category_weight)
        self.box_weight = float(DEFAULT_BOX_WEIGHT if box_weight is None else box_weight)
        self.attribute_weight = float(DEFAULT_ATTRIBUTE_WEIGHT if attribute_weight is None else attribute_weight)
        self.exist_weight = float(DEFAULT_EXIST_WEIGHT if exist_weight is None else exist_weight)
        self.MatchingMask = MatchingMask()
        self.loss_scale = 1.0            # 1/num_replicas under data parallelism
        self.last_match: Optional[torch.Tensor] = None
        self.last_cost: Optional[torch.Tensor] = None
        self.last_num_objects: Optional[torch.Tensor] = None
        self.built = True

    def call(self, inputs, training=False):
        """The predictions may hold several calls stacked along the batch axis ([L * B, N, ...] against targets of B images: the decoder
        layers' heads under DETR(use_intermediate_losses=True)): cost matrix, assignment and loss then run once over all L * B images,
        every block of B images being one loss call of its own, and `losses` is [6][L * B]."""
        y_true, y_pred = inputs
        category, attribute, bbox, num_objects = y_true
        cat_preds, attribute_preds, box_preds = y_pred
        B, N, Cc = cat_preds.shape
        M = category.shape[1]
        A = attribute_preds.shape[-1]
        period = category.shape[0] if category.shape[0] != B else None
        d = K.loss_desc(B, M, N, Cc, A, self.category_weight, self.attribute_weight, self.box_weight, self.exist_weight)
        cost = K.cost_matrix(d, cat_preds, attribute_preds, box_preds, category, attribute, bbox, num_objects, period=period)
        match = K.lsa(cost, num_objects, period=period)
        tape = current_tape()
        losses, d_cat, d_att, d_box = K.set_loss(d, cat_preds, attribute_preds, box_preds, category, attribute, bbox,
                                                 num_objects, match, loss_scale=self.loss_scale, want_grads=tape is not None, period=period)
        self.last_match, self.last_cost, self.last_num_objects = match, cost, num_objects
        if tape is not None:
            tape.record([losses], [cat_preds, attribute_preds, box_preds], lambda g: (d_cat, d_att, d_box))
        total, cat_l, att_l, box_l, exist_l, iou = (losses[i] for i in range(6))
        self._losses_tensor = losses
        return [total, cat_l, att_l, box_l, exist_l], [iou]

    def __call__(self, inputs, training=False, **kw):
        return self.call(inputs, training=training)


class MatchingMetric(Layer):
    """IoU of matched pairs (176-192) - computed inside MatchingLoss's kernel; kept for API parity."""

    def __init__(self, name="MatchingMetric", **kwargs):
        super().__init__(name=name, **kwargs)
        self.built = True


class MaskLoss(Layer):
    """Mask loss of the panoptic head (DETR(train_panoptic_head=True)).  The reference defines none (its model.py:4 leaves the
    head out), so this is the DETR paper's: sigmoid focal loss (alpha .25, gamma 2; TFA sigmoid_focal_crossentropy from logits,
    averaged over the pixels) + DICE, per matched (object m -> query n) pair of the last decoder layer's assignment
    (``MatchingLoss.last_match``; masks are not part of the matching cost), summed over the objects and divided by
    max(num_objects, 1), times ``mask_weight``.

    ``call(masks_pred [B,N,P], masks [B,M,P] (or [B,M,h,w]), match int32 [B,M], num_objects int32 [B])`` -> loss [B].  When a
    Tape is recording, the kernel's gradient (``loss_scale`` x dloss/dlogits, zero rows for unmatched queries) is registered."""

    def __init__(self, mask_weight=1.0, name="MaskLoss", **kwargs):
        super().__init__(name=name, **kwargs)
        self.mask_weight = float(mask_weight)
        self.loss_scale = 1.0
        self.built = True

    @staticmethod
    def check_targets(masks, B: int, M: int, P: int) -> torch.Tensor:
        if masks is None:
            raise ValueError(f"train_panoptic_head needs inputs['masks'] ([B, M, h, w] or [B, M, h*w] with B={B}, M={M}, h*w={P})")
        shape = tuple(masks.shape)
        if not (len(shape) in (3, 4) and shape[:2] == (B, M) and math.prod(shape[2:]) == P):
            raise ValueError(f"inputs['masks'] has shape {shape}; expected [B, M, h, w] or [B, M, h*w] with B={B}, M={M}, h*w={P}")
        return masks

    def call(self, masks_pred, masks, match, num_objects, training=False):
        B, N, P = masks_pred.shape
        tape = current_tape()
        loss, dlogits = K.mask_loss(masks_pred, masks.reshape(B, -1, P), match, num_objects, self.mask_weight, self.loss_scale,
                                    want_grads=tape is not None)
        if tape is not None:
            tape.record([loss], [masks_pred], lambda g: (dlogits,))
        return loss

    def __call__(self, masks_pred, masks, match, num_objects, training=False, **kw):
        return self.call(masks_pred, masks, match, num_objects, training=training)
