"""Panoptic head (drop-in for /root/reference/ModelComponents/panoptic_neck.py:8-186; its attention input comes from
transformers.PanopticAttention, transformers.py:460-559).

The reference never wires these layers into a model (the import is commented out, model.py:4) and never trains them.  Here
the head runs frozen and forward-only by default (``DETR.panoptic_masks``); with ``DETR(train_panoptic_head=True)`` it runs
inside the training step on the Tape and learns from ``MaskLoss`` (losses_and_metrics.py).
Channel counts shrink / grow by 2/3 and 3/2 (100 -> 66 -> 44 -> 29 ...), so tensors carry their TRUE channel count
next to a storage width padded to a multiple of 4 (zeros): ``(tensor [B,H,W,ld], C)``.  Convolutions run on the MFMA
implicit-GEMM kernels with zero-padded weights, packed from the Keras-layout variables on the device at every forward
(a pure copy; no host round trip inside a step); Conv2DTranspose(k=2, stride 1, valid) is the full-padding convolution
with the taps flipped and the in/out axes of the Keras kernel swapped.

Every op below records its backward on the current Tape (when one is recording).  Parameter gradients go through
``ops.GradSink`` (the conv weight gradients inside ``side_task``), activation gradients return through the Tape."""
from __future__ import annotations

import numpy as np
import torch

from . import kernels as K
from .engine import Layer, current_tape, side_task
from .ops import GradSink, own, _rec

LN_EPS = 1e-3            # tf.keras.layers.LayerNormalization default
LEAKY = 0.01             # ReLU(negative_slope=.01)
MASK_GRID = 23           # output grid: Resizing(96, 96) -> ... -> ConvOut(k=3, s=4): 94 -> 23


def _view(x: torch.Tensor, shape) -> torch.Tensor:
    """x.view(shape) linked to x on the Tape (the Tape keys on tensor identity)."""
    y = x.view(shape)
    _rec([y], [x], lambda g: (g.reshape(x.shape),))
    return y


def conv_packed(x: torch.Tensor, kernel, bias, transpose: bool, stride: int, pad: int) -> torch.Tensor:
    """Conv2D (HWIO kernel) / Conv2DTranspose (as a pad-1 conv with flipped taps) of a channel-padded NHWC tensor."""
    w, b = K.conv_weight_pack(kernel.value, bias.value, transpose)
    N, H, W, ld = x.shape
    assert w.shape[-1] == ld, (w.shape, x.shape)
    geom = K.ConvGeom(N, H, W, ld, w.shape[0], w.shape[1], w.shape[2], stride, pad)
    y, _ = K.conv2d_fwd(x, w, b, geom, K.ACT_NONE)
    if current_tape() is None:
        return y

    def backward(g):
        g = g.contiguous()
        if kernel.needs_grad or bias.needs_grad:
            def param_grads(g=g):
                dw = K.conv2d_bwd_weight(x, g, geom)
                db = K.colsum(g.view(-1, g.shape[-1]))
                sk = GradSink(kernel) if kernel.needs_grad else None
                sb = GradSink(bias) if bias.needs_grad else None
                K.conv_weight_unpack(dw, db, kernel.keras_shape, transpose, sk.buf if sk else None, sb.buf if sb else None)
                for sink in (sk, sb):
                    if sink is not None:
                        sink.commit()
            side_task(param_grads, x, g, w)
        return (own(K.conv2d_bwd_data(g, w, geom)),)

    _rec([y], [x], backward)
    return y


def layernorm_act(y: torch.Tensor, C: int, gamma, beta, slope: float) -> torch.Tensor:
    out = K.layernorm_act(y, C, gamma.value, beta.value, LN_EPS, slope)
    if current_tape() is None:
        return out

    def backward(g):
        sg, sb = GradSink(gamma), GradSink(beta)
        dy, _, _ = K.layernorm_act_bwd(y, C, gamma.value, beta.value, LN_EPS, slope, g.contiguous(), dgamma=sg.buf, dbeta=sb.buf)
        sg.commit()
        sb.commit()
        return (own(dy),)

    _rec([out], [y], backward)
    return out


def resize_bilinear(x: torch.Tensor, H: int, W: int) -> torch.Tensor:
    y = K.resize_bilinear(x, H, W)
    _rec([y], [x], lambda g: (own(K.resize_bilinear_bwd(g.contiguous(), x.shape[1], x.shape[2])),))
    return y


def concat(parts):
    """Concatenate (tensor, C) pairs along the TRUE channels into one padded tensor; the backward slices the columns back out."""
    C = sum(c for _, c in parts)
    t0 = parts[0][0]
    out = torch.empty(tuple(t0.shape[:-1]) + (K.pad4(C),), dtype=torch.float32, device=t0.device)
    if K.pad4(C) != C:
        K.zero_(out)
    col = 0
    for t, c in parts:
        assert t.shape[:-1] == t0.shape[:-1], (t.shape, t0.shape)
        K.copy_cols(t, c, out, col)
        col += c
    if current_tape() is None:
        return out, C

    def backward(g):
        g = g.contiguous()
        gins, col = [], 0
        for t, c in parts:
            d = K.empty(*t.shape, like=g)
            if t.shape[-1] != c:
                K.zero_(d)
            gins.append(own(K.copy_cols(g, c, d, 0, src_col0=col)))
            col += c
        return tuple(gins)

    _rec([out], [t for t, _ in parts], backward)
    return out, C


def nhwc_to_nchw(y: torch.Tensor, C: int) -> torch.Tensor:
    N, H, W, ld = y.shape
    out = K.nhwc_to_nchw(y, C)
    _rec([out], [y], lambda g: (own(K.nchw_to_nhwc(g.contiguous(), H, W, ld)),))
    return out


class _ConvLNBlock(Layer):
    """num_repeats x [Conv2D / Conv2DTranspose (k=2) -> LayerNormalization -> leaky ReLU]; filters *= 2/3 or 3/2."""

    transpose = False

    def __init__(self, num_repeats=2, name=None, **kwargs):
        super().__init__(name=name, **kwargs)
        self.num_repeats = num_repeats

    def get_config(self):
        c = super().get_config()
        c.update({"num_repeats": self.num_repeats})
        return c

    def next_filters(self, f: int) -> int:
        return 3 * f // 2 if self.transpose else 2 * f // 3

    def build(self, input_shape):
        self.features_shape = input_shape[0]
        f = self.in_channels
        self.convs = []
        for i in range(self.num_repeats):
            g = self.next_filters(f)
            keep, self.name = self.name, f"{self.name}/Conv2D_{i}"
            kshape = (2, 2, g, f) if self.transpose else (2, 2, f, g)          # Conv2DTranspose kernels are [kh, kw, out, in]
            kernel = self.add_weight("kernel", kshape, "glorot_uniform")
            bias = self.add_weight("bias", (g,), "zeros")
            self.name = f"{keep}/LayerNormalization_{i}"
            gamma, beta = self.add_weight("gamma", (g,), "ones"), self.add_weight("beta", (g,), "zeros")
            self.name = keep
            self.convs.append((kernel, bias, gamma, beta, f, g))
            f = g
        self.out_channels = f

    def __call__(self, inputs, training=False, **kw):
        x, C = inputs[0]
        if not self.built:
            self.in_channels = C
            self.build([tuple(x.shape)])
            self.built = True
        return self.call(inputs, training=training)

    def call(self, inputs, training=False):
        x, C = inputs[0]
        for kernel, bias, gamma, beta, f, g in self.convs:
            y = conv_packed(x, kernel, bias, self.transpose, 1, 1 if self.transpose else 0)
            x = layernorm_act(y, g, gamma, beta, LEAKY)
        return x, self.out_channels


class DownscaleBlock(_ConvLNBlock):
    """panoptic_neck.py:91-135."""
    transpose = False


class UpscaleBlock(_ConvLNBlock):
    """panoptic_neck.py:138-186."""
    transpose = True


class PanopticNeck(Layer):
    """panoptic_neck.py:8-88.  call([features [B,rows,cols,num_obj,dim]]) -> [B, num_obj, 23*23]."""

    def __init__(self, name="PanopticNeck", **kwargs):
        super().__init__(name=name, **kwargs)

    def build(self, input_shapes):
        self.features_shape = input_shapes[0]
        self.num_obj = self.features_shape[3]
        p = f"{self.scope}/"
        mk = lambda cls, n, nm: cls(num_repeats=n, name=nm, scope_prefix=p)
        self.DownscaleBlock_0, self.DownscaleBlock_1 = mk(DownscaleBlock, 1, "DownscaleBlock_0"), mk(DownscaleBlock, 1, "DownscaleBlock_1")
        self.DownscaleBlock_2, self.DownscaleBlock_3 = mk(DownscaleBlock, 2, "DownscaleBlock_2"), mk(DownscaleBlock, 3, "DownscaleBlock_3")
        self.UpscaleBlock_0, self.UpscaleBlock_1 = mk(UpscaleBlock, 3, "UpscaleBlock_0"), mk(UpscaleBlock, 2, "UpscaleBlock_1")
        self.UpscaleBlock_2, self.UpscaleBlock_3 = mk(UpscaleBlock, 1, "UpscaleBlock_2"), mk(UpscaleBlock, 2, "UpscaleBlock_3")
        self.DownscaleBlock_4 = mk(DownscaleBlock, 1, "DownscaleBlock_4")

    _concat = staticmethod(concat)

    def call(self, inputs, training=False):
        features = inputs[0]                                   # [B, rows, cols, num_obj, dim]
        B, r, c = features.shape[:3]
        C = int(np.prod(features.shape[3:]))
        x = _view(features.contiguous(), (B, r, c, C))         # ReshapeInput
        if K.pad4(C) != C:
            x, _ = self._concat([(x, C)])
        orig = (resize_bilinear(x, 96, 96), C)                 # Resize
        d0 = self.DownscaleBlock_0([orig])
        d1 = self.DownscaleBlock_1([d0])
        d2 = self.DownscaleBlock_2([d1])
        d3 = self.DownscaleBlock_3([d2])
        u0 = self.UpscaleBlock_0([d3])
        join_a = self._concat([u0, d2])
        u1 = self.UpscaleBlock_1([u0])
        join_b = self._concat([u1, d1])
        u2 = self.UpscaleBlock_2([u1])
        join_c = self._concat([u2, d0])
        join_a = self.UpscaleBlock_3([join_a])
        join_c = self.DownscaleBlock_4([join_c])
        feats, cin = self._concat([join_a, join_b, join_c])
        if not hasattr(self, "ConvOut_kernel"):
            keep, self.name = self.name, f"{self.name}/ConvOut"
            self.ConvOut_kernel = self.add_weight("kernel", (3, 3, cin, self.num_obj), "glorot_uniform")
            self.ConvOut_bias = self.add_weight("bias", (self.num_obj,), "zeros")
            self.name = keep
        y = conv_packed(feats, self.ConvOut_kernel, self.ConvOut_bias, False, 4, 0)     # ConvOut: k=3, strides=4, valid
        return nhwc_to_nchw(y, self.num_obj)                   # TransposeOut + FlattenDim: [B, num_obj, OH*OW]
