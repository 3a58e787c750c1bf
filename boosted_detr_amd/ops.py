"""Tape-recorded composite ops of the hot path.  Each function runs HIP kernels for the
forward and, when a Tape is recording, registers the closure that runs the backward kernels.

Activation gradients travel through the Tape; PARAMETER gradients do not: each backward
closure writes them straight into the variable's slice of the optimizer's flat gradient buffer
(``GradSink``), so there is no per-tensor staging copy before the all-reduce / optimizer.

Tensors are NHWC / [B,T,D]; ops view them as 2-D row matrices internally.
"""
from __future__ import annotations

import math
import os
import weakref
from typing import Optional

import numpy as np
import torch

from . import kernels as K
from . import _lib
from .engine import WEIGHTS_VERSION, Variable, capture, current_tape, dense_contribution, info, materialise, own, side_task, tag

# Dropout masks are keyed by (per-step seed, dropout site, element index).  The per-step seed lives in HBM
# (one int64 the host rewrites before every step), the site salt is a launch argument: a captured step graph then
# draws fresh masks on every replay.
_dropout_site = [0]
_dropout_seed_dev = [None]


def dropout_seed_tensor() -> torch.Tensor:
    if _dropout_seed_dev[0] is None:
        _dropout_seed_dev[0] = torch.full((1,), 0x5EED, dtype=torch.int64, device="cuda")
    return _dropout_seed_dev[0]


def set_dropout_seed(seed: int, write: bool = True) -> None:
    """Start a step: reset the site counter and (unless a graph replay already staged it) store the step's seed."""
    if write:
        dropout_seed_tensor().fill_(int(seed) & 0x7FFFFFFFFFFF)
    _dropout_site[0] = 0


def _next_dropout_seed() -> int:
    _dropout_site[0] += 1
    return (_dropout_site[0] * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


def _rec(outputs, inputs, fn):
    t = current_tape()
    if t is not None:
        t.record(outputs, inputs, fn)


def _2d(t: torch.Tensor) -> torch.Tensor:
    return t.view(-1, t.shape[-1])


_live_flat_grad = [None]


def set_live_flat_grad(flat: Optional[torch.Tensor]) -> None:
    """The flat gradient buffer that was zero-filled for THIS step (Model.forward_backward), or None.  A
    Variable.grad_buf is only written in place when it is a slice of exactly this buffer: after compile(new
    optimizer) or a freeze/unfreeze cycle a variable may still carry a slice of a retired buffer that holds an
    earlier step's gradients, and the split-K atomics would add onto them."""
    _live_flat_grad[0] = flat


_grad_ready_hook = [None]


def set_grad_ready_hook(fn) -> None:
    """fn(var) is called after every gradient contribution to a parameter has been enqueued (data-parallel training
    launches a bucket's all-reduce once all of its gradients are complete and live in the flat buffer)."""
    _grad_ready_hook[0] = fn


class GradSink:
    """Where a backward kernel writes one parameter's gradient.

    direct: first contribution of the step and the variable owns a slice of the flat buffer zeroed this step -> in place.
    temp  : later contribution (shared layer), no optimizer yet, or a stale slice -> temporary, added on commit.
    drop  : the variable is frozen but the kernel always produces the value -> scratch."""

    __slots__ = ("var", "buf", "mode")

    def __init__(self, var: Variable):
        self.var = var
        live = _live_flat_grad[0]
        if not var.needs_grad:
            self.mode, self.buf = "drop", torch.empty_like(var.value)
        elif var.grad is None and var.grad_buf is not None and live is not None and getattr(var, "_grad_flat", None) is live:
            self.mode, self.buf = "direct", var.grad_buf      # zero-filled at the start of the step (Model.forward_backward)
        else:
            self.mode, self.buf = "temp", torch.empty_like(var.value)

    def commit(self) -> None:
        v = self.var
        if self.mode == "direct":
            v.grad, v._grad_fresh = v.grad_buf, True
        elif self.mode == "temp":
            if v.grad is None:
                v.grad = self.buf
            else:
                K.axpy_(1.0, self.buf.view(v.grad.shape), v.grad)
        if self.mode != "drop" and _grad_ready_hook[0] is not None:
            _grad_ready_hook[0](v)


# ----------------------------------------------------------------------------------------
# backbone
# ----------------------------------------------------------------------------------------
def image_prep(image: torch.Tensor, H: int, W: int) -> torch.Tensor:
    return K.image_prep(image, H, W)     # input images need no gradient


COMPACT_S2 = os.environ.get("BDETR_COMPACT_S2", "1") != "0"       # stride-2 1x1 input gradients as compact even-pixel tensors (_p16_input_grad)


class BNState:
    """gamma/beta/moving stats of one BatchNormalization layer + its hyper-parameters."""

    def __init__(self, gamma: Variable, beta: Variable, moving_mean: Variable, moving_var: Variable, eps: float,
                 momentum: float = 0.99):
        self.gamma, self.beta, self.moving_mean, self.moving_var = gamma, beta, moving_mean, moving_var
        self.eps, self.momentum = eps, momentum


def _bn_forward(y2d, rows, Cc, parts, bn: BNState, use_batch_stats: bool, bessel: bool, residual2d, relu: bool):
    if use_batch_stats:
        if parts is None or parts[0] is None:
            parts = K.colstats(y2d)
        mean, rstd = K.bn_stats(rows, Cc, parts, bn.eps, bn.momentum, bessel, bn.moving_mean.value, bn.moving_var.value, like=y2d)
    else:
        K.demote_split_forward()
        mean, rstd = K.bn_stats_frozen(bn.moving_mean.value, bn.moving_var.value, bn.eps)
    out = K.bn_apply(y2d, mean, rstd, bn.gamma.value, bn.beta.value, residual2d, relu)
    return out, mean, rstd


def _bn_backward(g2d, out2d, x2d, mean, rstd, bn: BNState, relu: bool, frozen: bool, want_residual_grad: bool):
    sg, sb = GradSink(bn.gamma), GradSink(bn.beta)
    # without a residual the ReLU mask is a function of x alone: the kernel recomputes it instead of reading `out`
    mask_src = out2d if (relu and want_residual_grad) else None
    dx, _, _, dres = K.bn_bwd(g2d, mask_src, x2d, mean, rstd, bn.gamma.value, relu, frozen, want_residual_grad=want_residual_grad,
                              dgamma=sg.buf, dbeta=sb.buf, beta=bn.beta.value)
    sg.commit()
    sb.commit()
    return dx, dres


# ---- pre-split (P16) operand path of the backbone convolutions (csrc/sgemm.hip) ----
# Under the 'split' policy a training-mode Conv+BN unit whose channel counts allow it runs on operands that their
# producers already wrote as 16-bit pairs: BatchNorm apply writes the f16 pair (forward operand of the next conv)
# and the bf16 pair (its weight-gradient operand), BatchNorm backward writes the bf16 pair of dy, the weights are
# packed once per optimizer step.  A tensor handle carries its packed companions in an ActInfo record (below).
P16_ENABLED = [os.environ.get("BDETR_P16", "1") != "0"]
# The weight gradient reads the f16 pair the FORWARD of its convolution read (converted to bf16 pairs inside the kernel,
# bdetr_p16_conv2d_bwd_weight_xf16), so activations have no bf16 pair copy at all: bn_apply_p16 writes 4 bytes per element less.
WGRAD_XF16 = os.environ.get("BDETR_WGRAD_XF16", "1") != "0"
BF16_FOR_3X3 = os.environ.get("BDETR_BF16_3X3", "1") != "0"       # ... except in front of a 3x3 convolution (conv_bn want_bf16)
EVEN_PIXELS = os.environ.get("BDETR_EVEN_PIXELS", "1") != "0"  # stage-last BatchNorm backward reduces over the even pixels only (_p16_bn_backward)
EVEN_APPLY = os.environ.get("BDETR_EVEN_APPLY", "1") != "0"    # stage-last BatchNorm apply writes the even pixels only (_conv_bn_p16)
LAZY_SKIP = os.environ.get("BDETR_LAZY_SKIP", "1") != "0"      # residual units hand their skip gradient on unmasked (_p16_bn_backward)
BN_FUSE = os.environ.get("BDETR_BN_FUSE", "1") != "0"          # BatchNorm-backward sums in the consumer's backward-data epilogue (ActInfo.bn_ctx, bn_ctx_bits)
BN_FUSE2 = os.environ.get("BDETR_BN_FUSE2", "1") != "0"        # ... also those of a deferred projection-shortcut BatchNorm (ActInfo.bn_ctx_bits2)


def _p16_active() -> bool:
    return P16_ENABLED[0] and K.get_gemm_precision() == "split"


# ---- what a conv_bn output handle carries forward for its consumers ----
class ActInfo:
    """Packed companions and BatchNorm contexts of an activation handle; hangs on the tensor as `_act_info`.  A record never holds the
    tensor it hangs on, nor a view of it (see conv_bn_relu_maxpool): that would be a reference cycle the GC collects late or never."""
    # f16 / bf16     P16-f16 / P16-bf16 copies (fp32-shaped torch tensors, never read as floats)
    # p16_only       the handle IS the f16 copy: no fp32 tensor was materialised (links inside a bottleneck)
    # deferred_bn    (mean, rstd, gamma, beta): the handle is a projection shortcut's RAW convolution output, its BatchNorm still to apply
    # bn_ctx         (y, mean, rstd, gamma, beta, relu) of the BatchNorm that wrote a link with exactly one consumer (the next conv of the
    #                bottleneck): that conv's backward-data epilogue can do THIS BatchNorm's backward reduction while it stores the gradient
    # bn_ctx_bits    (y, mean, rstd, gamma, beta, relu bit mask) of a residual unit whose output gradient the next unit's skip merge completes
    # bn_ctx_bits2   (raw shortcut output, mean, rstd) of that unit's deferred projection-shortcut BatchNorm: it gets the same gradient
    __slots__ = ("f16", "bf16", "p16_only", "deferred_bn", "bn_ctx", "bn_ctx_bits", "bn_ctx_bits2")

    def __init__(self):
        self.p16_only = False
        self.f16 = self.bf16 = self.deferred_bn = self.bn_ctx = self.bn_ctx_bits = self.bn_ctx_bits2 = None


_NO_ACT = ActInfo()         # shared by every untagged tensor (and None): read-only


def act_info(t) -> ActInfo:
    return getattr(t, "_act_info", _NO_ACT)


def _act_tag(t: torch.Tensor) -> ActInfo:
    a = getattr(t, "_act_info", None)
    if a is None:
        a = t._act_info = ActInfo()
    return a


def attach_packed(t: torch.Tensor, f16: torch.Tensor, bf16: Optional[torch.Tensor] = None, p16_only: bool = False) -> torch.Tensor:
    """Hang the packed copies of activation `t` on its handle (p16_only: `t` has no fp32 values, `f16` is all there is)."""
    a = _act_tag(t)
    a.f16, a.bf16, a.p16_only = f16, bf16, p16_only
    return t


def is_p16_only(t: torch.Tensor) -> bool:
    return act_info(t).p16_only


def as_fp32(t: torch.Tensor) -> torch.Tensor:
    """The fp32 tensor behind a handle (unpacks a P16-only handle: 2^-23 relative round trip; applies a deferred
    BatchNorm: conv_bn(defer_apply=True))."""
    a = act_info(t)
    if a.p16_only:
        return K.p16_unpack(a.f16, True).view(t.shape)
    if a.deferred_bn is not None:
        return K.bn_apply(_2d(t), *a.deferred_bn, None, False).view(t.shape)
    return t


def _packed_input(x: torch.Tensor, need_bf16: bool):
    """(f16 pair, bf16 pair | None) of an activation, packing an fp32 handle once and caching the result on it."""
    a = act_info(x)
    xf, xb = a.f16, a.bf16
    need_bf16 = need_bf16 and not WGRAD_XF16
    if xf is None or (need_bf16 and xb is None):
        f, b = K.p16_pack(x, want_f16=xf is None, want_bf16=need_bf16 and xb is None)
        xf, xb = (f if xf is None else xf), (b if b is not None else xb)
        attach_packed(x, xf, xb, a.p16_only)
    return xf, xb


class _PackCache:
    """The two packed copies (forward operand, backward-data operand) of every weight matrix of one kind, in persistent buffers,
    refreshed by ONE multi-tensor launch the first time a copy is asked for after the weights changed (optimizer step / assign).
    The table keeps the buffers of its rows alive; rows of variables that no longer exist are dropped whenever the table is rebuilt
    (a new variable registers).  alloc(value) -> the two buffers of a row; table_row(value, fwd, bwd) -> its int64 table row;
    pack(table) -> the launch that refreshes every row.  A Variable belongs to one cache (it carries its row as `_packs`)."""

    def __init__(self, alloc, table_row, pack):
        self.alloc, self.table_row, self.pack = alloc, table_row, pack
        self.rows, self.table, self.version = [], None, -1       # rows: (weakref(var), value, fwd copy, bwd copy)
        # tables a captured step launched its refresh with: the graph holds their ADDRESS, so they outlive the rebuild that a later
        # model's variables trigger (a second model built after a capture freed the table under the first one's replays)
        self.captured_tables = []

    def get(self, w: Variable):
        c = getattr(w, "_packs", None)
        if c is None or c[0].data_ptr() != w.value.data_ptr():
            c = w._packs = (w.value,) + self.alloc(w.value)
            self.rows = [r for r in self.rows if r[0]() is not None and r[0]() is not w]
            self.rows.append((weakref.ref(w),) + c)
            self.table, self.version = None, -1
        if self.version != WEIGHTS_VERSION[0]:
            if self.table is None:
                rows = np.array([self.table_row(*r[1:]) for r in self.rows], np.int64)
                self.table = torch.from_numpy(rows).to(w.value.device)
            self.pack(self.table)
            if capture() is not None and not any(t is self.table for t in self.captured_tables):
                self.captured_tables.append(self.table)
            self.version = WEIGHTS_VERSION[0]
        return c[1], c[2]


def _conv_pack_buffers(v: torch.Tensor):
    Kout, R, S, Cin = v.shape
    return torch.empty_like(v), torch.empty((Cin, R, S, Kout), dtype=torch.float32, device=v.device)


# conv kernels on the pre-split path: (P16-f16 forward copy [K,R,S,C], P16-bf16 transposed tap-flipped copy [C,R,S,K])
_PACKED = _PackCache(_conv_pack_buffers, lambda v, f, t: [v.data_ptr(), f.data_ptr(), t.data_ptr(), *v.shape],
                     K.p16_pack_conv_weights_multi)


def _write_param_grads(w: Variable, b: Variable, write_dw, bias_from: Optional[torch.Tensor]) -> None:
    """Weight, then bias gradient of a conv / dense unit into their GradSinks.  write_dw(buf, prezeroed) launches the weight gradient;
    the bias gradient is the column sum of the 2-D gradient `bias_from`, or - bias_from None - exactly zero: a bias in front of a
    batch-statistics BatchNorm, where sum_rows(dy) = -rstd*gamma*mean(g*xhat)*sum(xhat) and sum(xhat) == 0 (the fp64 oracle gives ~1e-15)."""
    if w.needs_grad:
        s = GradSink(w)
        write_dw(s.buf, s.mode == "direct")
        s.commit()
    if b.needs_grad:
        s = GradSink(b)
        if bias_from is not None:
            K.colsum(bias_from, out=s.buf, prezeroed=s.mode == "direct")
        elif s.mode != "direct":
            K.zero_(s.buf)
        s.commit()


def _param_grads_task(w: Variable, b: Variable, write_dw, bias_from: Optional[torch.Tensor], *keep) -> None:
    """_write_param_grads as one side task (`keep`: the operands the side stream reads, see engine.on_side_stream)."""
    if w.needs_grad or b.needs_grad:
        side_task(lambda: _write_param_grads(w, b, write_dw, bias_from), *keep)


def conv_bn(x: torch.Tensor, w: Variable, b: Variable, bn: BNState, stride: int, pad: int, relu: bool,
            residual: Optional[torch.Tensor] = None, training: bool = False, bn_batch_stats: Optional[bool] = None,
            x_needs_grad: bool = True, want_fp32: bool = True, want_p16: bool = False, defer_apply: bool = False,
            sole_consumer_is_identity_unit: bool = False, consumers_read_even_pixels: bool = False, want_bf16: bool = False) -> torch.Tensor:
    """Conv2D(+bias) -> BatchNormalization -> [+ residual] -> [ReLU]  (keras ResNet-50 block unit).

    sole_consumer_is_identity_unit (residual units): the only consumers of this output are the next unit's first 1x1
    convolution and its identity skip - the masked accumulate that completes this output's gradient there can then also do
    THIS unit's BatchNorm-backward reduction (ctx attached to the handle as `bn_ctx_bits`).
    consumers_read_even_pixels (a stage's last unit): the only consumers of this output are stride-2 1x1 convolutions, which read the
    pixels (2i, 2j) and nothing else - on the pre-split path with a P16-only output on an even map with C % 256 == 0 the BatchNorm apply
    pass then reads and writes those pixels alone (EVEN_APPLY).  The handle keeps its full [N, H, W, C] shape; its other pixels, and
    their ReLU mask words, hold whatever the allocation held.  Everything else takes the dense pass.
    defer_apply (projection shortcut, no ReLU, no residual; P16 path only): the statistics are reduced but the normalised
    tensor is not written - the returned handle is the RAW convolution output tagged `deferred_bn`, and the unit that takes
    it as `residual` applies both BatchNorms in its one pass (bn_apply_p16 residual_bn; as_fp32 is the fallback).

    want_p16: the consumer is another conv_bn - also emit the packed copy of the output (P16 path only): the f16 pair, which feeds
    the consumer's forward AND (converted in registers) its weight gradient; want_bf16: additionally a bf16 pair copy for that weight
    gradient - worth its 4 bytes per element only for the quarter-width tensor in front of a 3x3 convolution;
    want_fp32=False: no fp32 output at all, the returned handle is the f16 copy (valid on the P16 path only,
    otherwise ignored)."""
    N, H, W, Cin = x.shape
    Kout, R, S, _ = w.value.shape
    g = K.ConvGeom(N, H, W, Cin, Kout, R, S, stride, pad)
    use_batch = training if bn_batch_stats is None else bn_batch_stats
    if training and use_batch and _p16_active() and K.p16_supported(g):
        return _conv_bn_p16(x, w, b, bn, g, relu, residual, x_needs_grad, want_fp32, want_p16, defer_apply, sole_consumer_is_identity_unit,
                            consumers_read_even_pixels, want_bf16)
    return _conv_bn_fp32(x, w, b, bn, g, relu, residual, use_batch, x_needs_grad)


def _conv_bn_fp32(x, w: Variable, b: Variable, bn: BNState, g, relu: bool, residual, use_batch: bool, x_needs_grad: bool) -> torch.Tensor:
    """conv_bn on the plain fp32 kernels (inference, moving statistics, policies and geometries without a pre-split kernel)."""
    x32 = as_fp32(x)
    res2d = _2d(as_fp32(residual)) if residual is not None else None
    y, parts = K.conv2d_fwd(x32, w.value, b.value, g, K.ACT_NONE, want_stats=use_batch)
    y2d = _2d(y)
    out2d, mean, rstd = _bn_forward(y2d, g.M, g.K, parts, bn, use_batch, True, res2d, relu)
    out = out2d.view(g.N, g.OH, g.OW, g.K)
    res_shape = residual.shape if residual is not None else None

    def backward(g_out, acc=None):
        return _conv_bn_backward_fp32(g_out, acc, x32, w, b, bn, g, relu, res_shape, use_batch, x_needs_grad, y2d, mean, rstd, out2d)

    backward.wants_acc = True
    backward.accepts_lazy = True
    _rec([out], [x, residual], backward)       # the Tape keys gradients by the handles their producers returned
    return out


def _conv_bn_backward_fp32(g_out, acc, x32, w: Variable, b: Variable, bn: BNState, g, relu: bool, res_shape, use_batch: bool,
                           x_needs_grad: bool, y2d, mean, rstd, out2d):
    """Backward of a Conv+BN unit on the plain fp32 kernels, from fp32 tensors (out2d: only read for the ReLU mask of a residual unit).
    Its kernels know none of the gradient tags: the incoming gradient is materialised."""
    g2d = _2d(materialise(g_out).contiguous())
    want_res = res_shape is not None
    dy, dres = _bn_backward(g2d, out2d, y2d, mean, rstd, bn, relu, not use_batch, want_res)
    dy4 = dy.view(g.N, g.OH, g.OW, g.K)
    _param_grads_task(w, b, lambda dw, pz: K.conv2d_bwd_weight(x32, dy4, g, dw=dw, prezeroed=pz), None if use_batch else dy, x32, dy)
    dx = None
    if x_needs_grad and acc is not None and acc[0] is not None:
        # residual merge fused into the GEMM epilogue: dx += conv_transpose(dy) (no separate add pass).  A compact even-pixel gradient
        # comes back from materialise as a NEW dense tensor: it replaces the offered one in `acc`, the Tape re-binds to it
        dx = acc[0] = materialise(acc[0])
        K.conv2d_bwd_data(dy4, w.value, g, dx=dx.view(g.N, g.H, g.W, g.C), accumulate=True)
        dense_contribution(dx)
    elif x_needs_grad:
        dx = own(K.conv2d_bwd_data(dy4, w.value, g))
    return dx, (own(dres.view(res_shape)) if want_res else None)


def _conv_bn_p16(x, w: Variable, b: Variable, bn: BNState, g, relu: bool, residual, x_needs_grad: bool, want_fp32: bool, want_p16: bool,
                 defer_apply: bool, sole_consumer_is_identity_unit: bool, consumers_read_even_pixels: bool, want_bf16: bool) -> torch.Tensor:
    """conv_bn on the pre-split operand path (training with batch statistics under the 'split' policy)."""
    ra = act_info(residual)
    res_p16, res_bn = ra.p16_only, ra.deferred_bn
    res2d = _2d(residual) if residual is not None else None     # a P16-only handle IS its f16 pair copy, a deferred one the RAW conv output
    xf, xb = _packed_input(x, need_bf16=w.needs_grad)
    y, parts = K.p16_conv2d_fwd(xf, _PACKED.get(w)[0], b.value, g, K.ACT_NONE, want_stats=True)
    y2d = _2d(y)
    mean, rstd = K.bn_stats(g.M, g.K, parts, bn.eps, bn.momentum, True, bn.moving_mean.value, bn.moving_var.value, like=y2d)
    fp32_out = want_fp32 or not want_p16
    # a residual unit without an fp32 output: its backward ReLU mask is a 1-bit-per-element by-product of this pass
    want_mask = relu and residual is not None and not fp32_out
    out2d = ob = relu_bits = None
    if defer_apply and not relu and residual is None:
        out = y.view(g.N, g.OH, g.OW, g.K)               # (a fresh handle: y itself stays this unit's own tensor)
        _act_tag(out).deferred_bn = (mean, rstd, bn.gamma.value, bn.beta.value)
    else:
        # the even-pixel pass: only where every reader of the output is known to take the pixels (2i, 2j) alone and the kernel admits the map
        even = (g.OH, g.OW) if (consumers_read_even_pixels and EVEN_APPLY and not fp32_out and g.OH % 2 == 0 and g.OW % 2 == 0
                                and g.K % 256 == 0) else None
        from . import engine as _engine
        # (diagnostic: engine.DebugLog fingerprints every layer's WHOLE output - the pixels the pass skips then hold zeros, not what the
        # allocation held, so that an eager step and its replay still log the same words)
        out2d, of, ob, *rest = K.bn_apply_p16(y2d, mean, rstd, bn.gamma.value, bn.beta.value, res2d, relu, want_fp32=fp32_out, want_f16=want_p16,
                                              want_bf16=want_p16 and ((want_bf16 and BF16_FOR_3X3) or not WGRAD_XF16), residual_p16=res_p16,
                                              want_mask=want_mask, residual_bn=res_bn, even_pixels=even,
                                              zero_unwritten=even is not None and _engine._DEBUG_LOG[0] is not None)
        relu_bits = rest[0] if want_mask else None
        out = (out2d if fp32_out else of).view(g.N, g.OH, g.OW, g.K)
    if want_p16:
        attach_packed(out, of.view(out.shape), ob.view(out.shape) if ob is not None else None, p16_only=not fp32_out)
    if relu_bits is not None and sole_consumer_is_identity_unit and BN_FUSE:
        _act_tag(out).bn_ctx_bits = (y2d, mean, rstd, bn.gamma.value, bn.beta.value, relu_bits)
        if res_bn is not None and BN_FUSE2:     # a stage's first unit: its sum(g * xhat0) rides the same epilogue
            _act_tag(out).bn_ctx_bits2 = (res2d, res_bn[0], res_bn[1])
    if not fp32_out and residual is None and BN_FUSE:
        _act_tag(out).bn_ctx = (y2d, mean, rstd, bn.gamma.value, bn.beta.value, relu)
    res_shape = residual.shape if residual is not None else None

    def backward(g_out, acc=None):
        if not _p16_active():
            # the backward runs under another arithmetic policy than the forward did (Model.replay_backward('fp32')): the fp32 kernels,
            # on the tensors this forward saved
            x32 = as_fp32(x)
            out32 = out2d if (out2d is not None or not (relu and residual is not None)) else _2d(as_fp32(out))
            return _conv_bn_backward_fp32(g_out, acc, x32, w, b, bn, g, relu, res_shape, True, x_needs_grad, y2d, mean, rstd, out32)
        dyb, dres = _p16_bn_backward(g_out, bn, g, relu, res_shape, res_bn, y2d, mean, rstd, out2d, relu_bits, ob)
        dyb4 = dyb.view(g.N, g.OH, g.OW, g.K)
        # the weight gradient's x operand: a bf16 pair copy where the producer wrote one, else the forward's f16 pair
        xw, xw_f16 = (xb, False) if xb is not None else (xf, True)
        _param_grads_task(w, b, lambda dw, pz: K.p16_conv2d_bwd_weight(xw, dyb4, g, dw=dw, prezeroed=pz, x_f16=xw_f16), None, xw, dyb)
        return (_p16_input_grad(dyb4, w, g, act_info(x), acc) if x_needs_grad else None), dres

    backward.wants_acc = True
    backward.accepts_lazy = True
    _rec([out], [x, residual], backward)       # the Tape keys gradients by the handles their producers returned
    return out


def _p16_bn_backward(g_out, bn: BNState, g, relu: bool, res_shape, res_bn, y2d, mean, rstd, out2d, relu_bits, ob):
    """BatchNorm(+residual, +ReLU) backward of a pre-split unit: (dy as its bf16 pair, the residual's gradient | None).  Reads the
    gradient tags its kernel knows (engine.GradInfo) and materialises the rest."""
    want_res, omap = res_shape is not None, (g.N, g.OH, g.OW)
    # A gradient that exists at the pixels (2i, 2j) only arrives as the compact [N, OH/2, OW/2, K] tensor its producers - the next stage's
    # stride-2 1x1 backward-data products (_p16_input_grad) - wrote densely: no zero-filled dense tensor, no scatter.  A residual unit reads
    # it through the pixel map in both of its consumers (this BatchNorm backward and the skip merge of the unit's first convolution);
    # every other case gets the dense form.
    gi = info(g_out)
    compact = gi.compact_even
    if compact is not None and not (relu and want_res and relu_bits is not None and LAZY_SKIP and compact == omap and gi.owned
                                    and gi.lazy_mask is None and gi.bnb_parts is None and g_out.is_contiguous()):
        g_out, compact = materialise(g_out), None
        gi = info(g_out)
    # g_out still needs its producer's ReLU mask (see lazy_skip below): only a BatchNorm with neither a ReLU nor a residual of its own
    # (a projection shortcut's) applies it in its kernel
    lazy_bits = gi.lazy_mask
    if lazy_bits is not None and (relu or want_res):
        g_out, lazy_bits = materialise(g_out), None
    g2d = _2d(g_out.contiguous())
    sg, sb = GradSink(bn.gamma), GradSink(bn.beta)
    # ReLU mask: recomputed from y when there is no residual, else the forward output (fp32), or - when that was never materialised in
    # fp32 - the bit mask bn_apply wrote (else the hi halves of the bf16 pair copy)
    mask_src, mode = None, 0
    if relu and want_res:
        mask_src, mode = (out2d, 0) if out2d is not None else ((relu_bits, 2) if relu_bits is not None else (ob, 1))
        assert mask_src is not None, "a residual unit without an fp32 output keeps its ReLU bit mask"
    pre = gi.bnb_parts                          # the reduction came with the gradient (fused into the consumer's epilogue)
    # The skip gradient of a residual unit is g_out * mask.  With the bit mask at hand it is not written out: the incoming gradient
    # tensor itself is handed to the shortcut's producer tagged with the mask, and the consumers that know the tag (the 1x1
    # backward-data of _p16_input_grad, the projection shortcut's BatchNorm backward) fold the mask into their own kernels - one
    # 4-byte-per-element write per unit less (engine.materialise is the fallback).
    lazy_skip = want_res and mode == 2 and LAZY_SKIP and gi.owned and lazy_bits is None and g_out.is_contiguous()
    bn_relu = relu
    if lazy_bits is not None:                   # this BatchNorm has no ReLU of its own: apply the incoming mask instead
        mask_src, mode, bn_relu = lazy_bits, 2, True
    even = gi.even_pixels if (EVEN_PIXELS and gi.even_pixels == omap) else None      # zero off the even pixels: a quarter-size reduction pass
    if compact is not None:
        assert lazy_skip and pre is None, "a compact even-pixel gradient is handed on to the skip merge as it is"
        even = compact
    dyb, _, _, _, dres = K.bn_bwd_p16(g2d, mask_src, y2d, mean, rstd, bn.gamma.value, bn_relu, False, want_residual_grad=want_res and not lazy_skip,
                                      dgamma=sg.buf, dbeta=sb.buf, beta=bn.beta.value, out_p16=mode, pre=pre, even_pixels=even,
                                      dout_compact=compact is not None)
    if lazy_skip:
        dres = own(g_out.view(res_shape) if compact is None else g_out)      # (compact: keeps its `compact_even` tag)
        ri = tag(dres)
        ri.lazy_mask = relu_bits
        if gi.bnb_parts_shortcut is not None and res_bn is not None:
            ri.bnb_parts = gi.bnb_parts_shortcut      # the shortcut's BatchNorm backward finds its reduction done (it reads them as `pre`)
    elif want_res:
        dres = own(dres.view(res_shape))
    sg.commit()
    sb.commit()
    return dyb, (dres if want_res else None)


def _p16_input_grad(dyb4, w: Variable, g, xa: ActInfo, acc):
    """Input gradient of a pre-split convolution.  Which backward-data kernel runs depends on what is already accumulated for x
    (acc[0], offered by the Tape: accumulate into it, or put the tensor that replaces it there) and on what the handle of x (`xa`)
    asks its consumer's epilogue to reduce.  The ORDER of the cases is part of the behaviour."""
    N, H, W, Cin = g.N, g.H, g.W, g.C
    imap = (N, H, W)
    one = g.R == 1 and g.S == 1 and g.pad == 0
    s1, s2 = one and g.stride == 1, one and g.stride == 2
    # a stride-2 1x1 convolution's input gradient lives at the pixels (2i, 2j): on an even map it is produced as the compact
    # [N, H/2, W/2, C] tensor - a plain dense product over the OUTPUT grid - and tagged; see _p16_bn_backward
    s2c = s2 and COMPACT_S2 and H % 2 == 0 and W % 2 == 0
    gc = K.ConvGeom(N, g.OH, g.OW, Cin, g.K, 1, 1, 1, 0) if s2c else None
    keep_even = imap if s2 else None            # (an even-pixel tag survives further stride-2 1x1 contributions on its map)
    _, wt = _PACKED.get(w)
    have = acc[0] if acc is not None else None
    hi = info(have)
    if hi.compact_even is not None:
        if s2c and hi.compact_even == imap and hi.lazy_mask is None:
            # the other stride-2 consumer of x was first: add into its compact tensor
            K.p16_conv2d_bwd_data(dyb4, wt, gc, dx=have.view(N, g.OH, g.OW, Cin), accumulate=True)
            return have
        if hi.lazy_mask is not None and s1 and hi.compact_even == imap and xa.bn_ctx_bits2 is None:
            # the skip merge of a stage's last unit: conv_transpose(dy) + expand(compact gradient) * mask into a FRESH dense tensor
            # (+ the previous unit's BatchNorm-backward sums, when its handle asks for them)
            dx = acc[0] = own(K.empty(N, H, W, Cin, like=dyb4))
            r = K.p16_conv2d_bwd_data_masked_accum(dyb4, wt, g, dx, hi.lazy_mask, bn_ctx=xa.bn_ctx_bits, old_even=have)
            if xa.bn_ctx_bits is not None:
                tag(dx).bnb_parts = r[1]
            return dx
        # a compact tensor meets anything else: the dense form (a new tensor), then the plain accumulate
        dx = acc[0] = materialise(have)
        K.p16_conv2d_bwd_data(dyb4, wt, g, dx=dx.view(N, H, W, Cin), accumulate=True)
        dense_contribution(dx, keep_even)
        return dx
    if have is not None:
        dense_contribution(have, keep_even)
        if hi.lazy_mask is not None and s1:
            # masked accumulate: the skip merge of a residual unit in this epilogue.  Where it completes the previous unit's output
            # gradient it does that unit's BatchNorm-backward sums too, and those of its projection shortcut's BatchNorm
            r = K.p16_conv2d_bwd_data_masked_accum(dyb4, wt, g, have.view(N, H, W, Cin), hi.lazy_mask, bn_ctx=xa.bn_ctx_bits,
                                                   bn_ctx2=xa.bn_ctx_bits2)
            if xa.bn_ctx_bits is not None:
                hi.bnb_parts = r[1]
                if xa.bn_ctx_bits2 is not None:
                    hi.bnb_parts_shortcut = r[2]
            hi.lazy_mask = None
        else:
            K.p16_conv2d_bwd_data(dyb4, wt, g, dx=materialise(have).view(N, H, W, Cin), accumulate=True)
        return have
    if xa.bn_ctx is not None and g.stride == 1:
        # fresh, with the BatchNorm-backward sums of the producer of x
        dx, parts = K.p16_conv2d_bwd_data_bnstats(dyb4, wt, g, *xa.bn_ctx)
        tag(dx).bnb_parts = parts
    elif s2c:
        dx = K.p16_conv2d_bwd_data(dyb4, wt, gc)
        tag(dx).compact_even = imap
    else:
        # a dense stride-2 1x1 gradient is zero-filled, then written at the pixels (2i, 2j) only: the tag lets the producer's BatchNorm
        # backward reduce over those pixels alone
        dx = K.p16_conv2d_bwd_data(dyb4, wt, g)
        if s2:
            tag(dx).even_pixels = imap
    return own(dx)


def conv_act(x: torch.Tensor, w: Variable, b: Variable, stride: int, pad: int, act: int) -> torch.Tensor:
    """Conv2D + bias + activation (BackboneNeck.conv2d_downscaler: 1x1, tanh)."""
    N, H, W, Cin = x.shape
    Kout, R, S, _ = w.value.shape
    g = K.ConvGeom(N, H, W, Cin, Kout, R, S, stride, pad)
    y, _ = K.conv2d_fwd(x, w.value, b.value, g, act)

    def backward(g_out):
        g_out = g_out.contiguous()
        if act == K.ACT_TANH:
            dpre = K.tanh_bwd(y, g_out)
        elif act == K.ACT_RELU:
            dpre = K.relu_bwd(y, g_out)
        else:
            dpre = g_out
        _param_grads_task(w, b, lambda dw, pz: K.conv2d_bwd_weight(x, dpre, g, dw=dw, prezeroed=pz), _2d(dpre), x, dpre)
        return (own(K.conv2d_bwd_data(dpre, w.value, g)),)

    _rec([y], [x], backward)
    return y


def batchnorm(x: torch.Tensor, bn: BNState, training: bool, bessel: bool) -> torch.Tensor:
    """Stand-alone BatchNormalization over the last axis (neck: 4-D fused path -> bessel moving
    variance; heads: 3-D path -> biased)."""
    x2d = _2d(x)
    rows, Cc = x2d.shape
    out2d, mean, rstd = _bn_forward(x2d, rows, Cc, None, bn, training, bessel, None, False)
    out = out2d.view(x.shape)

    def backward(g_out):
        dx, _ = _bn_backward(_2d(g_out.contiguous()), None, x2d, mean, rstd, bn, False, not training, False)
        return (own(dx.view(x.shape)),)

    _rec([out], [x], backward)
    return out


def batchnorm_rows(x: torch.Tensor, bn: BNState, training: bool, groups: int) -> torch.Tensor:
    """BatchNormalization of `groups` stacked calls: x is [groups * B, ..., C] and every [B, ..., C] block is normalised with its own batch
    statistics (biased variance: the heads' 3-D keras path), the moving statistics updated once per block in block order
    (csrc/groupnorm_rows.hip).  One statistics + one apply launch forward, two launches backward, one contribution to gamma / beta."""
    x2d = _2d(x)
    g, b = bn.gamma.value, bn.beta.value
    if training:
        mean, rstd, var = K.bn_rows_stats(x2d, groups, bn.eps)
        out2d = K.bn_rows_apply(x2d, groups, mean, rstd, g, b, var, bn.momentum, bn.moving_mean.value, bn.moving_var.value)
    else:
        K.demote_split_forward()
        mean, rstd = K.bn_stats_frozen(bn.moving_mean.value, bn.moving_var.value, bn.eps)
        out2d = K.bn_rows_apply(x2d, groups, mean, rstd, g, b)
    out = out2d.view(x.shape)

    def backward(g_out):
        sg, sb = GradSink(bn.gamma), GradSink(bn.beta)
        dx, _, _ = K.bn_rows_bwd(_2d(g_out.contiguous()), x2d, groups, mean, rstd, bn.gamma.value, not training, dgamma=sg.buf, dbeta=sb.buf)
        sg.commit()
        sb.commit()
        return (own(dx.view(x.shape)),)

    _rec([out], [x], backward)
    return out


def stack_rows(xs) -> torch.Tensor:
    """[B, N, D] x L -> [L * B, N, D] (the decoder layers' outputs in front of the shared heads).  The backward hands every input its own
    [B, N, D] block of the incoming gradient; the Tape adds it to what the next decoder block sends."""
    L, B = len(xs), xs[0].shape[0]
    out = torch.empty((L * B,) + tuple(xs[0].shape[1:]), dtype=xs[0].dtype, device=xs[0].device)
    for l, x in enumerate(xs):
        K.copy_cols(x.contiguous(), x.shape[-1], out[l * B:(l + 1) * B], 0)

    def backward(g):
        # the blocks are disjoint and nothing else reads an owned g behind this node: each block is then the Tape's own
        g, mine = g.contiguous(), info(g).owned
        return tuple(own(g[l * B:(l + 1) * B]) if mine else g[l * B:(l + 1) * B] for l in range(L))

    _rec([out], list(xs), backward)
    return out


def maxpool(x: torch.Tensor) -> torch.Tensor:
    y = K.maxpool_fwd(x)
    _rec([y], [x], lambda g: (own(K.maxpool_bwd(x, y, g.contiguous())),))
    return y


STEM_FUSE = os.environ.get("BDETR_STEM_FUSE", "1") != "0"
STEM_S2D = os.environ.get("BDETR_STEM_S2D", "1") != "0"            # the stem's weight gradient on the pre-split path (conv_bn_relu_maxpool backward)


def conv_bn_relu_maxpool(x: torch.Tensor, w: Variable, b: Variable, bn: BNState, stride: int, pad: int, training: bool,
                         bn_batch_stats: bool) -> torch.Tensor:
    """The ResNet stem: Conv2D(+bias) -> BatchNormalization -> ReLU -> ZeroPadding2D(1) -> MaxPool 3x3/2; the input image needs no
    gradient.  Training with batch statistics under the 'split' policy, the tail runs fused (csrc/norm.hip stem_*): the pooled tensor is
    written once, as the f16 pair its consumers read (the returned handle IS that copy, like a link inside a bottleneck), and the
    normalised full-resolution tensor and its gradient are never materialised.  Otherwise: conv_bn + maxpool."""
    N, H, W, Cin = x.shape
    Kout, R, S, _ = w.value.shape
    if not (STEM_FUSE and training and bn_batch_stats and _p16_active() and Kout % 8 == 0):
        return maxpool(conv_bn(x, w, b, bn, stride, pad, True, training=training, bn_batch_stats=bn_batch_stats, x_needs_grad=False))
    g = K.ConvGeom(N, H, W, Cin, Kout, R, S, stride, pad)
    x32 = as_fp32(x)
    y, parts = K.conv2d_fwd(x32, w.value, b.value, g, K.ACT_NONE, want_stats=True)
    if parts is None or parts[0] is None:
        parts = K.colstats(_2d(y))
    mean, rstd = K.bn_stats(g.M, Kout, parts, bn.eps, bn.momentum, True, bn.moving_mean.value, bn.moving_var.value, like=y)
    _, out, tap = K.stem_pool_fwd(y, mean, rstd, bn.gamma.value, bn.beta.value)
    # `out` IS the f16 pair copy.  The alias must not lead back to `out`: `out` itself is a cycle through its own __dict__ (freed only by
    # the cyclic GC: 105 MB per step at batch 16), and a VIEW is worse - its C-level `_base` edge is invisible to the GC, so the cycle
    # out -> view -> out is never collected (that leaked 100 MB per eager step: profiles/r05_soak_2000steps_eager_leak.txt).
    # detach() shares the storage and holds no reference to the tensor object.
    attach_packed(out, out.detach(), p16_only=True)

    def backward(g_out):
        sg, sb = GradSink(bn.gamma), GradSink(bn.beta)
        # The weight gradient of the 7x7 / stride-2 / pad-3 stem over a 4-channel image with even sides runs on the pre-split XX kernel
        # through a space-to-depth view (kernels.stem_bwd_weight_s2d): it is the LAST kernel of the backward pass, alone on the chip
        # with the optimizer waiting for it.  dy is then written as its bf16 pair.  Gradient products under 'split' are bf16 pairs on
        # both paths; any other backward policy, deterministic mode and other geometries keep igemm.hip's kernel.
        s2d = (STEM_S2D and w.needs_grad and (R, S, stride, pad, Cin) == (7, 7, 2, 3, 4) and H % 2 == 0 and W % 2 == 0 and Kout % 64 == 0
               and K.get_gemm_precision() in ("split", "mixed") and not K.deterministic())
        dy, _, _ = K.stem_pool_bwd(materialise(g_out).contiguous(), tap, y, mean, rstd, bn.gamma.value, bn.beta.value, dgamma=sg.buf, dbeta=sb.buf,
                                   dy_p16=s2d)
        sg.commit()
        sb.commit()
        if s2d:
            _param_grads_task(w, b, lambda dw, pz: K.stem_bwd_weight_s2d(x32, dy, dw), None, x32, dy)
        else:
            _param_grads_task(w, b, lambda dw, pz: K.conv2d_bwd_weight(x32, dy, g, dw=dw, prezeroed=pz), None, x32, dy)
        return (None,)

    _rec([out], [x], backward)
    return out


# ----------------------------------------------------------------------------------------
# dense / elementwise
# ----------------------------------------------------------------------------------------
def dense(x: torch.Tensor, w: Variable, b: Variable, act: int = K.ACT_NONE) -> torch.Tensor:
    """tf.keras.layers.Dense on the last axis; w is stored [out][in]."""
    x2d = _2d(x)
    y2d = K.linear_fwd(x2d, w.value, b.value, act)
    y = y2d.view(*x.shape[:-1], w.value.shape[0])

    def backward(g_out, acc=None):
        g2d = _2d(g_out.contiguous())
        if act == K.ACT_RELU:
            g2d = K.relu_bwd(y2d, g2d)
        elif act == K.ACT_TANH:
            g2d = K.tanh_bwd(y2d, g2d)
        _param_grads_task(w, b, lambda dw, pz: K.linear_bwd_weight(g2d, x2d, dw=dw, prezeroed=pz), g2d, x2d, g2d)
        have = acc[0] if acc is not None else None
        if have is not None and have.is_contiguous() and have.shape == x.shape:
            # another consumer's gradient of x is already there: add into it in the GEMM epilogue (no separate axpy pass)
            K.linear_bwd_data(g2d, w.value, dx=_2d(materialise(have)), accumulate=True)
            dense_contribution(have)
            return (have,)
        return (own(K.linear_bwd_data(g2d, w.value).view(x.shape)),)

    backward.wants_acc = True
    _rec([y], [x], backward)
    return y


def dense_group(xs, ws, bs):
    """Independent Dense layers of identical width (the Q/K/V projections of an attention block,
    transformers.py:68-70) as ONE grouped GEMM launch forward and one for the input gradients."""
    x2 = [_2d(x) for x in xs]
    aligned = all(t.data_ptr() % 16 == 0 for t in x2) and x2[0].shape[1] % 4 == 0 and ws[0].value.shape[0] % 4 == 0
    same = all(w.value.shape == ws[0].value.shape for w in ws)
    if not (aligned and same) or len(xs) > 4:
        return [dense(x, w, b) for x, w, b in zip(xs, ws, bs)]
    y2 = K.linear_fwd_group(x2, [w.value for w in ws], [b.value for b in bs])
    ys = [y.view(*x.shape[:-1], y.shape[1]) for y, x in zip(y2, xs)]

    def backward(*gs):
        g2 = [_2d(g.contiguous()) for g in gs]

        def param_grads():
            # weight gradients of the projections that share a shape go out as one grouped split-K launch (self-attention: all three;
            # cross-attention: key + value, the query projection has its own row count)
            groups = {}
            for g, x, w in zip(g2, x2, ws):
                if w.needs_grad:
                    groups.setdefault((tuple(g.shape), tuple(x.shape)), []).append((g, x, GradSink(w)))
            for members in groups.values():
                K.linear_bwd_weight_group([m[0] for m in members], [m[1] for m in members], [m[2].buf for m in members], [m[2].mode == "direct" for m in members])
                for m in members:
                    m[2].commit()
            # bias gradients: the members whose sink is a zero-filled slice of the flat gradient buffer share ONE launch
            sinks = [(g, GradSink(b)) for g, b in zip(g2, bs) if b.needs_grad]
            direct = [(g, s) for g, s in sinks if s.mode == "direct"]
            if len(direct) > 1 and not K.deterministic() and all(g.shape[1] == direct[0][0].shape[1] for g, _ in direct):
                K.colsum_group([g for g, _ in direct], [s.buf for _, s in direct])
                for _, s in direct:
                    s.commit()
                sinks = [(g, s) for g, s in sinks if s.mode != "direct"]
            for g, s in sinks:
                K.colsum(g, out=s.buf, prezeroed=s.mode == "direct")
                s.commit()
        if any(w.needs_grad or b.needs_grad for w, b in zip(ws, bs)):
            side_task(param_grads, *x2, *g2)
        dxs = K.linear_bwd_data_group(g2, [w.value for w in ws])
        return tuple(own(dx.view(x.shape)) for dx, x in zip(dxs, xs))

    _rec(ys, list(xs), backward)
    return ys


def add(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    out = K.add(a, b)
    _rec([out], [a, b], lambda g: (g, g))        # shared tensor: NOT owned
    return out


def _param_or_tensor_grad(p, fn):
    """Gradient of a broadcast operand that may be a Variable's value (positional table, queries)."""
    if isinstance(p, Variable):
        if p.needs_grad:
            s = GradSink(p)
            fn(s.buf)
            s.commit()
        return None
    return fn(None)


def add_bcast(x: torch.Tensor, row) -> torch.Tensor:
    """x [B, ...] + row [...]  (positional encoding tiled over the batch, transformers.py:299-300).
    ``row`` is a tensor or a Variable."""
    rv = row.value if isinstance(row, Variable) else row
    out = K.add_bcast_rows(x, rv)
    n = rv.numel()

    def backward(g):
        g = g.contiguous()
        grow = _param_or_tensor_grad(row, lambda out_: K.sum_over_batch(g, n, out=out_))
        return g, (grow.view(rv.shape) if grow is not None else None)

    _rec([out], [x, None if isinstance(row, Variable) else row], backward)
    return out


def tile_batch(row: Variable, B: int) -> torch.Tensor:
    """row [...] -> [B, ...]  (DecoderPrep's tiled queries, transformers.py:445-447)."""
    rv = row.value
    zeros = torch.empty((B,) + tuple(rv.shape), dtype=rv.dtype, device=rv.device)
    K.zero_(zeros)
    out = K.add_bcast_rows(zeros, rv)
    n = rv.numel()
    from . import engine as _engine
    if _engine._DEBUG_LOG[0] is not None:
        _engine._DEBUG_LOG[0].emit("L", out)        # diagnostic: the zero-filled + broadcast tensor (see bdetr_zero_bytes)

    def backward(g):
        g = g.contiguous()
        _param_or_tensor_grad(row, lambda out_: K.sum_over_batch(g, n, out=out_))
        return ()

    _rec([out], [], backward)
    return out


def reshape(x: torch.Tensor, shape) -> torch.Tensor:
    y = x.view(shape)

    def backward(g):
        r = g.contiguous().view(x.shape)
        return (own(r) if info(g).owned else r,)

    _rec([y], [x], backward)
    return y


# ----------------------------------------------------------------------------------------
# transformer pieces
# ----------------------------------------------------------------------------------------
def attention_core(Q: torch.Tensor, Kt: torch.Tensor, V: torch.Tensor, heads: int, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """softmax(Q K^T / sqrt(d)) V per head (transformers.py:86-97).  Q [B,q,h*d], K/V [B,k,h*d].
    Returns [B,h,q,d] contiguous - the layout the reference reshapes WITHOUT permuting (line 100).

    mask (optional): [B or 1, h or 1, q or 1, k], contiguous, on the operands' device.  float32: the reference's rule (line 94),
    (softmax(S) * mask) V, nothing renormalised.  bool: exclusion, True attends, a False key takes no part in the softmax; a row
    with no kept key gives zeros and zero gradients.  The mask is a constant: the backward returns gradients for Q, K and V only.
    mask=None is the path, the kernels and the bits of a call without the keyword."""
    B, q, D = Q.shape
    kk = Kt.shape[1]
    d = D // heads
    scale = 1.0 / math.sqrt(float(d))
    if d == 32 and FUSED_ATTENTION[0]:
        O, lse = K.attention_fwd(Q, Kt, V, heads, scale, mask=mask)

        def backward_fused(gO):
            dQ, dK, dV = K.attention_bwd(Q, Kt, V, O, gO.contiguous(), lse, heads, scale, mask=mask)      # (the mask: a constant, no gradient)
            return own(dQ), own(dK), own(dV)

        _rec([O], [Q, Kt, V], backward_fused)
        return O
    if mask is not None:
        K._attention_mask_args(mask, B, heads, q, kk, Q)      # a bad mask is a ValueError before the first launch
    exclude = mask is not None and mask.dtype == torch.bool
    S = K.empty(B, heads, q, kk, like=Q)
    K.gemm_raw(q, kk, d, Q, D, True, Kt, D, True, S, kk, nb0=B, nb1=heads, sa=(q * D, d), sb=(kk * D, d), sc=(heads * q * kk, q * kk))
    if exclude:                                   # excluded scores: a large finite negative (a row with no kept key stays finite) ...
        K.attention_mask_apply(S, mask, fill=True, out=S)
    P = K.softmax_rows_fwd(S.view(-1, kk), scale, out=S.view(-1, kk)).view(B, heads, q, kk)   # in place; Rescaling is fused
    PM = P                                        # what multiplies V: P, P with the excluded keys zeroed, or P * mask
    if exclude:
        K.attention_mask_apply(P, mask, out=P)    # ... and their probabilities are exact zeros afterwards (an empty row: all zeros)
    elif mask is not None:
        PM = K.attention_mask_apply(P, mask)      # the softmax backward needs the unmasked P: P * mask is a second tensor
    O = K.empty(B, heads, q, d, like=Q)
    K.gemm_raw(q, d, kk, PM, kk, True, V, D, False, O, d, nb0=B, nb1=heads, sa=(heads * q * kk, q * kk), sb=(kk * D, d), sc=(heads * q * d, q * d))

    def backward(gO):
        gO = gO.contiguous()
        sP, sO = (heads * q * kk, q * kk), (heads * q * d, q * d)
        # dP[q][k] = sum_d dO[q][d] V[k][d]
        dP = K.empty(B, heads, q, kk, like=Q)
        K.gemm_raw(q, kk, d, gO, d, True, V, D, True, dP, kk, nb0=B, nb1=heads, sa=sO, sb=(kk * D, d), sc=sP, grad=True)
        if mask is not None:
            K.attention_mask_apply(dP, mask, out=dP)          # multiply: dP = M * (dO V^T); exclusion: zero at the excluded keys
        # dV[k][d] = sum_q P[q][k] dO[q][d]   (P * mask under the multiply rule)
        dV = K.empty(B, kk, D, like=Q)
        K.gemm_raw(kk, d, q, PM, kk, False, gO, d, False, dV, D, nb0=B, nb1=heads, sa=sP, sb=sO, sc=(kk * D, d), grad=True)
        dS = K.softmax_rows_bwd(P.view(-1, kk), dP.view(-1, kk), scale, out=dP.view(-1, kk)).view(B, heads, q, kk)
        # dQ[q][d] = sum_k dS[q][k] K[k][d] ;  dK[k][d] = sum_q dS[q][k] Q[q][d]
        dQ = K.empty(B, q, D, like=Q)
        K.gemm_raw(q, d, kk, dS, kk, True, Kt, D, False, dQ, D, nb0=B, nb1=heads, sa=sP, sb=(kk * D, d), sc=(q * D, d), grad=True)
        dK = K.empty(B, kk, D, like=Q)
        K.gemm_raw(kk, d, q, dS, kk, False, Q, D, False, dK, D, nb0=B, nb1=heads, sa=sP, sb=(q * D, d), sc=(kk * D, d), grad=True)
        return own(dQ), own(dK), own(dV)

    _rec([O], [Q, Kt, V], backward)
    return O


FUSED_ATTENTION = [True]     # head dim 32 -> csrc/attention.hip; other widths use batched GEMMs + softmax


def add_dropout_layernorm(x: torch.Tensor, y: torch.Tensor, gamma: Variable, beta: Variable, eps: float, rate: float,
                          training: bool) -> torch.Tensor:
    """LayerNormalization(x + Dropout(y))  (transformers.py:135-137, 178-180)."""
    r = rate if training else 0.0
    seed = _next_dropout_seed() if r > 0.0 else 0
    x2d, y2d = _2d(x), _2d(y)
    base = dropout_seed_tensor() if r > 0.0 else None
    out2d, mean, rstd = K.add_dropout_layernorm_fwd(x2d, y2d, gamma.value, beta.value, eps, r, seed, seed_base=base)
    out = out2d.view(x.shape)

    def backward(g_out):
        sg, sb = GradSink(gamma), GradSink(beta)
        dx, dy, _, _ = K.add_dropout_layernorm_bwd(_2d(g_out.contiguous()), x2d, y2d, gamma.value, mean, rstd, r, seed,
                                                   dgamma=sg.buf, dbeta=sb.buf, seed_base=base)
        sg.commit()
        sb.commit()
        return own(dx.view(x.shape)), own(dy.view(y.shape))

    _rec([out], [x, y], backward)
    return out


# ----------------------------------------------------------------------------------------
# row chain: OutputProjection + Add/Dropout/LayerNorm (+ FeedForwardBlock) of a transformer layer as one launch per direction
# ----------------------------------------------------------------------------------------
ROWCHAIN = [os.environ.get("BDETR_ROWCHAIN", "1") != "0"]


def rowchain_active(width: int) -> bool:
    """The fused path exists for model width 256 under the 'split' policy (csrc/rowchain.hip: f16-pair forward, bf16-pair gradient
    products); every other case runs the separate GEMM / LayerNorm launches."""
    return ROWCHAIN[0] and width == K.ROWCHAIN_WIDTH and K.get_gemm_precision() == "split"


def _rowchain_pack_buffers(v: torch.Tensor):
    n = int(_lib.lib().bdetr_rowchain_pack_elems())
    return torch.empty(n, dtype=torch.float32, device=v.device), torch.empty(n, dtype=torch.float32, device=v.device)


# Dense kernels on a row chain: (f16 pairs of 2^8 W in MFMA fragment order, bf16 pairs of W^T)
_RC_PACKED = _PackCache(_rowchain_pack_buffers, lambda v, f, t: [v.data_ptr(), f.data_ptr(), t.data_ptr()],
                        K.rowchain_pack_weights)


def attention_out_chain(ctx: torch.Tensor, resid: torch.Tensor, out_proj, ln1, ffn, eps: float, rate: float, training: bool) -> torch.Tensor:
    """LN1(resid + Dropout(ctx Wo^T + bo)) and, with ``ffn`` = (W1, b1, W2, b2, gamma2, beta2), the FeedForwardBlock behind it
    (transformers.py:101,135-137,174-180) as ONE forward launch; the backward closure runs one launch for every data gradient, LayerNorm
    gradient and bias gradient of the chain, one for their partial sums, and the three weight gradients as side tasks.
    out_proj = (Wo, bo), ln1 = (gamma1, beta1): Variables.  ctx, resid: [B, T, 256]."""
    r = rate if training else 0.0
    seed1 = _next_dropout_seed() if r > 0.0 else 0                  # the same site order as the unfused path: identical masks
    seed2 = _next_dropout_seed() if (r > 0.0 and ffn is not None) else 0
    base = dropout_seed_tensor() if r > 0.0 else None
    ctx2d, res2d = _2d(ctx.contiguous()), _2d(resid.contiguous())
    Wo, bo = out_proj
    g1, b1 = ln1
    ws = [Wo] + ([ffn[0], ffn[2]] if ffn is not None else [])
    bs = [bo] + ([ffn[1], ffn[3]] if ffn is not None else [])
    packs = [_RC_PACKED.get(w) for w in ws]
    saved = K.rowchain_fwd(ctx2d, res2d, [p[0] for p in packs], [b.value for b in bs], (g1.value, b1.value),
                           (ffn[4].value, ffn[5].value) if ffn is not None else None, eps, r, seed1, seed2, base)
    out = (saved["x2"] if ffn is not None else saved["x1"]).view(resid.shape)

    def backward_unfused(g_out):
        """The same backward on the separate kernels, from the tensors the fused forward saved - taken when the backward runs under
        another arithmetic policy than the forward did (Model.replay_backward('fp32'): exact-fp32 gradient products)."""
        g2 = _2d(g_out.contiguous())
        zeros = torch.zeros_like(ctx2d)                   # add_dropout_layernorm_bwd recomputes x + keep * y: x = the saved sum, y = 0
        todo = []
        if ffn is not None:
            W1, bb1, W2, bb2, g2v, b2v = ffn
            sg, sb = GradSink(g2v), GradSink(b2v)
            dh2, df, _, _ = K.add_dropout_layernorm_bwd(g2, saved["pre2"], zeros, g2v.value, saved["mean2"], saved["rstd2"], r, seed2,
                                                        dgamma=sg.buf, dbeta=sb.buf, seed_base=base)
            sg.commit(); sb.commit()
            dpre1 = K.relu_bwd(saved["h"], K.linear_bwd_data(df, W2.value))
            dx1 = K.linear_bwd_data(dpre1, W1.value, dx=dh2, accumulate=True)
            todo += [(W2, bb2, df, saved["h"]), (W1, bb1, dpre1, saved["x1"])]
        else:
            dx1 = g2
        sg, sb = GradSink(g1), GradSink(b1)
        dres, da, _, _ = K.add_dropout_layernorm_bwd(dx1, saved["pre1"], zeros, g1.value, saved["mean1"], saved["rstd1"], r, seed1,
                                                    dgamma=sg.buf, dbeta=sb.buf, seed_base=base)
        sg.commit(); sb.commit()
        dctx = K.linear_bwd_data(da, Wo.value)
        todo.append((Wo, bo, da, ctx2d))
        for w, b, g, x in todo:
            _write_param_grads(w, b, lambda dw, pz, g=g, x=x: K.linear_bwd_weight(g, x, dw=dw, prezeroed=pz), g)
        return own(dctx.view(ctx.shape)), own(dres.view(resid.shape))

    def backward(g_out):
        if K.get_gemm_precision() != "split":
            return backward_unfused(g_out)
        gammas = (g1.value,) + ((ffn[4].value,) if ffn is not None else ())
        packs_t = [_RC_PACKED.get(w)[1] for w in ws]
        dctx, dres, G, partials, nparts = K.rowchain_bwd(_2d(g_out.contiguous()), saved, packs_t, gammas, r, seed1, seed2, base)
        xs = [ctx2d] + ([saved["x1"], saved["h"]] if ffn is not None else [])
        vec_vars = ([ffn[4], ffn[5], ffn[3], ffn[1]] if ffn is not None else [None] * 4) + [g1, b1, bo]

        def param_grads():
            sinks = [GradSink(v) if v is not None else None for v in vec_vars]
            K.rowchain_reduce(partials, nparts, [s_.buf if s_ is not None else None for s_ in sinks], [0] * 7)
            for s_ in sinks:
                if s_ is not None:
                    s_.commit()
            todo = [(w, g, x, GradSink(w)) for w, g, x in zip(ws, G, xs) if w.needs_grad]
            if todo:                                           # the chain's weight gradients: one grouped split-K launch
                K.linear_bwd_weight_group([t[1] for t in todo], [t[2] for t in todo], [t[3].buf for t in todo], [t[3].mode == "direct" for t in todo])
                for t in todo:
                    t[3].commit()
        side_task(param_grads, partials, *G, *xs)
        return own(dctx.view(ctx.shape)), own(dres.view(resid.shape))

    _rec([out], [ctx, resid], backward)
    return out


# ----------------------------------------------------------------------------------------
# head activations
# ----------------------------------------------------------------------------------------
def softmax_lastdim(x: torch.Tensor) -> torch.Tensor:
    p = K.softmax_rows_fwd(_2d(x), 1.0).view(x.shape)
    _rec([p], [x], lambda g: (own(K.softmax_rows_bwd(_2d(p), _2d(g.contiguous()), 1.0).view(x.shape)),))
    return p


def sigmoid(x: torch.Tensor) -> torch.Tensor:
    y = K.sigmoid_fwd(x)
    _rec([y], [x], lambda g: (own(K.sigmoid_bwd(y, g.contiguous())),))
    return y


def box_sigmoid(x: torch.Tensor) -> torch.Tensor:
    """3*sigmoid(x/100) - 1  (prediction_heads.py:44)."""
    y = K.boxsigmoid_fwd(x)
    _rec([y], [x], lambda g: (own(K.boxsigmoid_bwd(y, g.contiguous())),))
    return y
