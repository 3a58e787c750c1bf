"""DETR model (drop-in for /root/reference/ModelComponents/model.py:12-244).

Same constructor signature, same ``call(inputs: dict, training)`` contract, same public sub-layer
attributes (EncoderBackbone, BackboneNeck, ImageEncoderAttention, DecoderPrep, DecoderBlocks[i],
CategoryPredictionHead, AttributePredictionHead, BoxPredictionHead, loss_fn), losses built into the
model (``add_loss`` of a per-image [B] vector, 5 ``add_metric`` calls), ``test_step`` == ``train_step``.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import backbone, losses_and_metrics, ops, prediction_heads, tokenizers, transformers
from . import kernels as K
from .engine import device, to_device
from .training import Model


def _prepare_targets(model, inputs):
    """model.py:148-158: tokenise strings (or accept ids) and move the targets to HBM."""
    category, attribute = model.Tokenization([inputs["category"], inputs["attribute"]])
    bbox = to_device(np.asarray(inputs["bbox"], np.float32) if not isinstance(inputs["bbox"], torch.Tensor) else inputs["bbox"])
    num_objects = inputs["num_objects"]
    num_objects = to_device(num_objects.reshape(-1) if isinstance(num_objects, torch.Tensor) else np.asarray(num_objects).reshape(-1), torch.int32)
    return [category, attribute, bbox, num_objects]


def _prepare_masks(inputs, B: int, M: int) -> torch.Tensor:
    """inputs["masks"]: float targets in [0, 1] on the head's 23 x 23 output grid, [B, M, 23, 23] or [B, M, 529], row m aligned with
    bbox row m (rows m >= num_objects[b] are ignored)."""
    from .panoptic_neck import MASK_GRID
    masks = losses_and_metrics.MaskLoss.check_targets(inputs.get("masks"), B, M, MASK_GRID * MASK_GRID)
    if not isinstance(masks, torch.Tensor):
        masks = np.asarray(masks, np.float32)
    return to_device(masks).reshape(B, M, MASK_GRID * MASK_GRID).contiguous()


def _inference_outputs(model, cat_preds, attribute_preds, box_coord_preds, raw: bool = False):
    """The tail of call(training=False), shared by DETR and BoostedDETR: the decoded strings of the reference, or
    with raw=True the three prediction tensors as they sit in HBM (Model.predict_raw)."""
    if raw:
        return [cat_preds, attribute_preds, box_coord_preds]
    category, attributes = model.InverseTokenization([cat_preds, attribute_preds], training=False)
    return category, attributes, box_coord_preds


def _image(inputs):
    img = inputs["image"]
    return to_device(img if isinstance(img, torch.Tensor) else np.asarray(img, np.float32))


VALID_REGION_KEY = "valid_region"


def check_valid_region(region, B: int, h: int, w: int, r: int, c: int, device=None):
    """inputs["valid_region"] against its contract, on the host and before anything is launched: int32 [B,4], rows (top, left,
    height, width) in pixels of the batch's h x w image as given.  Every failure is a ValueError.
    Every form: shape, dtype, and a device tensor on another device than `device` (None: not compared).
    A host array (a device tensor is never read back): top >= 0, left >= 0, height >= 1, width >= 1, the region inside the image,
    and at least one kept token per image on the r x c feature grid (kernels.token_keep_host, the kernel's integer rule).
    Returns the entry ready for to_device: the device tensor itself, or the host array as a contiguous int32 ndarray."""
    on_device = isinstance(region, torch.Tensor) and region.is_cuda
    if not on_device:
        region = region.numpy() if isinstance(region, torch.Tensor) else np.asarray(region)
    dtype_ok = region.dtype == (torch.int32 if on_device else np.int32)
    if not dtype_ok:
        raise ValueError(f"valid_region must be int32, got {region.dtype}")
    if tuple(region.shape) != (B, 4):
        raise ValueError(f"valid_region must be [B,4] = [{B},4] rows (top, left, height, width), got shape {tuple(region.shape)}")
    if on_device:
        if device is not None and region.device != device:
            raise ValueError(f"valid_region lives on {region.device}, the model on {device}")
        return region
    g = region.astype(np.int64)
    top, left, height, width = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
    for name, bad in (("top < 0", top < 0), ("left < 0", left < 0), ("height < 1", height < 1), ("width < 1", width < 1),
                      (f"top + height > {h}", top + height > h), (f"left + width > {w}", left + width > w)):
        if bad.any():
            b = int(np.argmax(bad))
            raise ValueError(f"valid_region[{b}] = {g[b].tolist()} of a {h} x {w} image: {name}")
    empty = ~K.token_keep_host(g, h, w, r, c).any(axis=1)
    if empty.any():
        b = int(np.argmax(empty))
        raise ValueError(f"valid_region[{b}] = {g[b].tolist()} of a {h} x {w} image holds no token centre of the {r} x {c} feature grid")
    return np.ascontiguousarray(region)


def _valid_region(model, inputs):
    """inputs["valid_region"] checked (check_valid_region; nothing launched yet) and in HBM with the image's (h, w), or None without the key."""
    region = inputs.get(VALID_REGION_KEY)
    if region is None:
        return None
    shape = tuple(np.shape(inputs["image"]))
    if len(shape) != 4:
        raise ValueError(f"valid_region needs an image [B,h,w,3], got shape {shape}")
    B, h, w = (int(s) for s in shape[:3])
    r, c = model.EncoderBackbone.feature_hw()
    return to_device(check_valid_region(region, B, h, w, r, c, device()), torch.int32), h, w


def _token_key_mask(valid_region, features):
    """The key mask [B,1,1,r*c] (bool, True attends) of the neck's output [B,r,c,D] for _valid_region's answer: one launch per call,
    on the device (include/bdetr.h K35), so a captured step follows the regions in its static input buffer.  None without the key."""
    if valid_region is None:
        return None
    region, h, w = valid_region
    return K.token_key_mask(region, h, w, int(features.shape[1]), int(features.shape[2]))


class DETR(Model):
    def __init__(self, num_object_preds, image_size, num_encoder_blocks, num_encoder_heads, encoder_dim,
                 num_decoder_blocks, num_decoder_heads, decoder_dim, num_panoptic_heads=1, panoptic_dim=32, vocab_dict=None,
                 classification_only=False, attribute_weight=1.0, name="DETR", **kwargs):
        seed = int(kwargs.pop("seed", 0))
        backbone_name = kwargs.pop("backbone_name", "ResNet")      # reference default is EfficientNet (out of scope)
        train_panoptic_head = bool(kwargs.pop("train_panoptic_head", False))
        with_panoptic_head = bool(kwargs.pop("with_panoptic_head", False)) or train_panoptic_head
        mask_weight = float(kwargs.pop("mask_weight", 1.0))
        use_intermediate_losses = bool(kwargs.pop("use_intermediate_losses", False))
        super().__init__(name=name, seed=seed)                      # pad_value / oov_value etc. are swallowed like the reference's **kwargs
        category_weight = box_weight = exist_weight = None
        if classification_only:
            box_weight = 0.0
        self.num_object_preds = num_object_preds
        self.image_size = tuple(image_size)
        self.num_encoder_blocks, self.num_encoder_heads, self.encoder_dim = num_encoder_blocks, num_encoder_heads, encoder_dim
        self.num_decoder_blocks, self.num_decoder_heads, self.decoder_dim = num_decoder_blocks, num_decoder_heads, decoder_dim
        self.num_panoptic_heads, self.panoptic_dim = num_panoptic_heads, panoptic_dim
        self.vocab_dict = vocab_dict

        self.Tokenization = tokenizers.Tokenization(vocab_dict=vocab_dict, name="Tokenization")
        self.InverseTokenization = tokenizers.InverseTokenization(vocab_dict=vocab_dict)
        sizes = self.Tokenization.vocab_size_dict()
        self.num_categories, self.num_attributes = sizes["category"], sizes["attributes"]

        self.EncoderBackbone = backbone.EncoderBackbone(image_input_shape=self.image_size, model_name=backbone_name,
                                                        name="EncoderBackbone", seed=seed)
        self.BackboneNeck = backbone.BackboneNeck(encoder_dim=encoder_dim, name="BackboneNeck", seed=seed)
        self.ImageEncoderAttention = transformers.ImageEncoderAttention(num_blocks=num_encoder_blocks, num_attention_heads=num_encoder_heads,
                                                                        name="ImageEncoderAttention", seed=seed)
        self.DecoderPrep = transformers.DecoderPrep(num_object_preds, decoder_dim, name="DecoderPrep", seed=seed)
        self.DecoderBlocks = [transformers.DecoderBlock_NoSelfAttention(num_attention_heads=num_decoder_heads, name="DecoderBlock_0", seed=seed)]
        for i in range(1, num_decoder_blocks):
            self.DecoderBlocks.append(transformers.DecoderBlock(num_attention_heads=num_decoder_heads, name=f"DecoderBlock_{i}", seed=seed))
        for b in self.DecoderBlocks:
            self.track(b)
        self.CategoryPredictionHead = prediction_heads.SingleClassPredictionHead(num_classes=self.num_categories, hidden_dim=4 * decoder_dim,
                                                                                 num_preds=num_object_preds, name="CategoryPredictionHead", seed=seed)
        self.AttributePredictionHead = prediction_heads.MultiClassPredictionHead(num_classes=self.num_attributes, hidden_dim=4 * decoder_dim,
                                                                                 num_preds=num_object_preds, name="AttributePredictionHead", seed=seed)
        self.BoxPredictionHead = prediction_heads.BoxPredictionHead(hidden_dim=decoder_dim, num_preds=num_object_preds,
                                                                    name="BoxPredictionHead", seed=seed)
        self.loss_fn = losses_and_metrics.MatchingLoss(category_weight=category_weight, box_weight=box_weight,
                                                       attribute_weight=attribute_weight, exist_weight=exist_weight, name="MatchingLoss")
        # BASELINE.json configs[4]'s mask head.  The reference constructs neither layer (model.py:4 has the import commented out;
        # num_panoptic_heads / panoptic_dim are accepted and unused), so the head is opt-in.  with_panoptic_head alone: forward-only
        # and frozen, it runs on the features the last call left behind (`panoptic_masks`), outside the training step's tape and
        # arithmetic policy.  train_panoptic_head (implies with_panoptic_head): the head runs inside call(training=True) on the
        # image encoding after the decoder loop, on the tape, and MaskLoss (weight mask_weight) joins the loss vector.
        self.train_panoptic_head = train_panoptic_head
        self.mask_weight = mask_weight
        self.PanopticAttention = self.PanopticNeck = self.MaskLoss = None
        if with_panoptic_head:
            from . import panoptic_neck
            self.PanopticAttention = transformers.PanopticAttention(num_attention_heads=num_panoptic_heads, hidden_dim=panoptic_dim, seed=seed)
            self.PanopticNeck = panoptic_neck.PanopticNeck(seed=seed)
            if train_panoptic_head:
                self.MaskLoss = losses_and_metrics.MaskLoss(mask_weight=mask_weight, name="MaskLoss")
            else:
                self.PanopticAttention.trainable = False
                self.PanopticNeck.trainable = False
        self._panoptic_inputs = None
        # Deep supervision (model.py:179,186: a switch the reference hard-codes to False): the shared heads, the matcher and the set loss
        # behind EVERY decoder block, the loss and the four loss metrics summed over the blocks; IOU, the returned predictions and
        # loss_fn.last_match stay the last block's.  May be changed between steps.  BDETR_AUX_STACKED=0 (read here) runs it as the
        # reference's per-block loop over the existing kernels instead of ONE pass of heads / matcher / loss over the stacked outputs.
        self.use_intermediate_losses = use_intermediate_losses
        self.aux_stacked = os.environ.get("BDETR_AUX_STACKED", "1") != "0"
        self.aux_predictions = None       # per decoder block [cat, att, box] of the last training call with the option on
        self.aux_logits = None            # ... and the three heads' pre-activation outputs
        self._aux_matches = None

    @property
    def aux_matches(self):
        """int32 [L, B, M]: every decoder block's assignment of the last training call with use_intermediate_losses, or None."""
        m = self._aux_matches
        return torch.stack(m) if isinstance(m, list) else m

    def _require_panoptic_head(self) -> None:
        if self.PanopticAttention is None:
            raise RuntimeError("construct the model with with_panoptic_head=True")

    def panoptic_masks(self):
        """[B, num_object_preds, 23 * 23] mask logits of the last call's images (transformers.py:460-559 on the image encoding +
        panoptic_neck.py:8-88), or None before the first call."""
        self._require_panoptic_head()
        if self._panoptic_inputs is None:
            return None
        enc, dec, pos = self._panoptic_inputs
        return self.PanopticNeck([self.PanopticAttention([enc, dec, pos])])

    def get_config(self):
        c = Model.get_config(self)            # explicit base: BoostedDETR reuses this function
        c.update({k: getattr(self, k) for k in ("num_object_preds", "image_size", "num_encoder_blocks", "num_encoder_heads", "encoder_dim",
                                                 "num_decoder_blocks", "num_decoder_heads", "decoder_dim", "num_panoptic_heads",
                                                 "panoptic_dim", "vocab_dict")})
        if getattr(self, "use_intermediate_losses", False):
            c["use_intermediate_losses"] = True
        return c

    def call(self, inputs, training=False, raw=False):
        """inputs["valid_region"] (optional; check_valid_region): the padding tokens are excluded as KEYS from the encoder's
        self-attention and from every decoder block's attention over the image (K33 / K35).  Without the key: the unmasked kernels."""
        valid_region = _valid_region(self, inputs)                # every refusal of the entry before anything is launched
        image = _image(inputs)
        if training:
            y_true = _prepare_targets(self, inputs)
            if self.train_panoptic_head:
                masks = _prepare_masks(inputs, image.shape[0], y_true[2].shape[1])

        encoder_features = self.EncoderBackbone([image], training=training)
        encoder_features = self.BackboneNeck([encoder_features], training=training)
        key_mask = _token_key_mask(valid_region, encoder_features)       # None without the key
        encoder_features, positional_encoding = self.ImageEncoderAttention([encoder_features], training=training, attention_mask=key_mask)
        image_encoding = encoder_features                         # [B, r, c, D]
        encoder_features, decoder_features, encoder_key, decoder_positional = \
            self.DecoderPrep([encoder_features, positional_encoding], training=training)

        use_intermediate_losses = bool(self.use_intermediate_losses)       # (hard-coded False in the reference, model.py:179)
        stacked = training and use_intermediate_losses and self.aux_stacked and self.num_decoder_blocks > 1
        loss_terms, metrics_i, y_pred_i = [], None, None
        layer_outputs, aux_preds, aux_logits, aux_matches = [], [], [], []
        for i in range(self.num_decoder_blocks):
            decoder_features = self.DecoderBlocks[i]([encoder_features, decoder_features, encoder_key, decoder_positional], training=training,
                                                     joint_attention_mask=key_mask)
            if stacked:
                layer_outputs.append(decoder_features)
            elif training and (use_intermediate_losses or i >= self.num_decoder_blocks - 1):
                cat_preds_i = self.CategoryPredictionHead([decoder_features], training=training)
                attribute_preds_i = self.AttributePredictionHead([decoder_features], training=training)
                box_coord_preds_i = self.BoxPredictionHead([decoder_features], training=training)
                y_pred_i = [cat_preds_i, attribute_preds_i, box_coord_preds_i]
                losses_i, metrics_i = self.loss_fn([y_true, y_pred_i])
                loss_terms.append(losses_i)
                self._loss_roots.append(self.loss_fn._losses_tensor)
                aux_preds.append(y_pred_i)
                aux_logits.append([h.last_logits for h in (self.CategoryPredictionHead, self.AttributePredictionHead, self.BoxPredictionHead)])
                aux_matches.append(self.loss_fn.last_match)
        if stacked:
            loss_terms, metrics_i, y_pred_i, aux_preds, aux_logits, aux_matches = self._stacked_heads_and_losses(layer_outputs, y_true)
        if training:
            self.aux_predictions, self.aux_logits, self._aux_matches = \
                (aux_preds, aux_logits, aux_matches) if use_intermediate_losses else (None, None, None)

        if self.PanopticAttention is not None:
            self._panoptic_inputs = (image_encoding, decoder_features, positional_encoding.value)
        mask_loss = None
        if training and self.train_panoptic_head:
            masks_pred = self.PanopticNeck([self.PanopticAttention([image_encoding, decoder_features, positional_encoding.value], training=training)],
                                           training=training)
            self.MaskLoss.mask_weight, self.MaskLoss.loss_scale = self.mask_weight, self.loss_fn.loss_scale
            mask_loss = self.MaskLoss(masks_pred, masks, self.loss_fn.last_match, y_true[3], training=training)
            self._loss_roots.append(mask_loss)
        if training:
            self._register(loss_terms, metrics_i, mask_loss)
            return y_pred_i

        cat_preds = self.CategoryPredictionHead([decoder_features], training=training)
        attribute_preds = self.AttributePredictionHead([decoder_features], training=training)
        box_coord_preds = self.BoxPredictionHead([decoder_features], training=training)
        return _inference_outputs(self, cat_preds, attribute_preds, box_coord_preds, raw)

    def _stacked_heads_and_losses(self, layer_outputs, y_true):
        """The shared heads, the matcher and the set loss behind every decoder block as ONE pass over the blocks' outputs stacked along
        the batch axis ([L * B, N, D]): every head GEMM, the cost matrix, the assignment (one workgroup per (block, image)) and the loss
        run once, BatchNormalization keeps each block's own batch statistics (ops.batchnorm_rows) and every head parameter receives one
        gradient contribution.  Returns what the per-block loop leaves: per-block loss terms, the last block's metrics / predictions,
        per-block predictions, logits and assignments (views of the stacked tensors)."""
        L, B = len(layer_outputs), layer_outputs[0].shape[0]
        features = ops.stack_rows(layer_outputs)
        heads = (self.CategoryPredictionHead, self.AttributePredictionHead, self.BoxPredictionHead)
        y_pred = [h([features], training=True, groups=L) for h in heads]
        losses, metrics = self.loss_fn([y_true, y_pred])
        self._loss_roots.append(self.loss_fn._losses_tensor)
        block = lambda t, l: t[l * B:(l + 1) * B]
        loss_terms = [[block(t, l) for t in losses] for l in range(L)]
        aux_preds = [[block(t, l) for t in y_pred] for l in range(L)]
        aux_logits = [[block(h.last_logits, l) for h in heads] for l in range(L)]
        for h in heads:
            h.last_logits = block(h.last_logits, L - 1)
        lf = self.loss_fn
        aux_matches = lf.last_match.view(L, B, -1)
        lf.last_match, lf.last_cost = block(lf.last_match, L - 1), block(lf.last_cost, L - 1)
        return loss_terms, [block(metrics[0], L - 1)], aux_preds[-1], aux_preds, aux_logits, aux_matches

    def _register(self, loss_terms, metrics_i, mask_loss=None):
        """model.py:206-221.  Per-learner loss vectors are kept as a list (summed on the host when
        logged) instead of being added on the device: the sum is never needed by the gradient.
        The panoptic head's mask loss (train_panoptic_head) is one more loss term and the Mask_Loss metric."""
        for k, name in enumerate(["loss", "Category_Loss", "Attribute_Loss", "Box_Loss", "Existence_Loss"]):
            terms = [t[k] for t in loss_terms]
            if name == "loss":
                for t in terms:
                    self.add_loss(t)
                if mask_loss is not None:
                    self.add_loss(mask_loss)
            else:
                self.add_metric(terms, name)
        self.add_metric([metrics_i[0]], "IOU")
        if mask_loss is not None:
            self.add_metric([mask_loss], "Mask_Loss")

    def citation(self):
        print("DETR-like model for object detection and fine-grained classification, after 'End-to-end Object Detection "
              "with Transformers' (Carion et al.); MI355X-native re-implementation of the mvenouziou/Boosted_DETR training path.")
